"""Times the nearest-point search (fi_nearest.hip) on the device; run it under rocprofv3 --kernel-trace for the per-kernel
times, then summarise the trace (profiles/nearest.md holds the numbers).  Queries and outputs live on the device (torch
tensors), so a query call is one k_nearest_query launch and nothing else.

    python tools/nearest_time.py config4 [side]   config 4's 1 M value points (bench.py --config 4) on its 256^3 lattice
    python tools/nearest_time.py config5 [side]   config 5's 5 M oriented points on its 512^3 lattice
    python tools/nearest_time.py summarize <kernel_trace.csv> <config4 / config5>

The phases, in this order: the structure built from the points (PointIndex, 1 + REPS times); the border prior on a fresh
context (fi_add_border_prior: border enumeration, a structure of its own, one query per border point), then the same prior
under FI_BORDER_BRUTE (the reference's loop over every pair); 1 M queries uniformly random over the lattice, then the same
queries sorted by lattice cell; the distance field of the whole lattice at max_distance = inf, then at 4.  `summarize` splits
the trace's launches of each kernel by that order and prints the medians.
"""
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 10
NQ = 1_000_000


def brute_reps(kind):
    return 1 if kind == "config5" else 3


def phases(kind):
    """[(label, kernel-name substring, launches)] in launch order (warm-up calls included: their first launch is dropped)"""
    return [("prior, tree: border queries", "k_nearest_query<3, 2>", 1 + REPS),
            ("prior, FI_BORDER_BRUTE: one launch per batch", "k_border_min_dist", brute_reps(kind)),
            ("prior, tree: the comparison's calls", "k_nearest_query<3, 2>", brute_reps(kind)),
            ("1 M random queries", "k_nearest_query<3, 0>", 1 + REPS),
            ("1 M sorted queries", "k_nearest_query<3, 0>", 1 + REPS),
            ("distance field, max_distance = inf", "k_nearest_query<3, 1>", 1 + REPS),
            ("distance field, max_distance = 4", "k_nearest_query<3, 1>", 1 + REPS)]


def points(kind, side):
    from field_interpolation_amd import synth
    if kind == "config4":
        side = side or 256
        sizes, w, pos, _ = synth.config4(side=side, num_points=int(round(1_000_000 * (side / 256.0) ** 3)), seed=3)
        return sizes, w, pos, None
    side = side or 512
    return synth.config5(side=side, num_points=int(round(5_000_000 * (side / 512.0) ** 2)), seed=4)


def wall(label, fn, reps):
    import torch
    fn()  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / reps
    print("%-46s %10.3f ms per call (wall)" % (label, ms))


def main(kind, side):
    import torch

    import field_interpolation_amd as fi
    sizes, w, pos, nrm = points(kind, side)
    n = len(pos)
    nb = int(np.prod(sizes) - np.prod([s - 2 for s in sizes]))
    print("%s: %d points, lattice %s, %d border points" % (kind, n, "x".join(map(str, sizes)), nb))
    pd = torch.from_numpy(pos).cuda()
    wall("build (PointIndex of the points)", lambda: fi.PointIndex(pd), REPS)

    def context():
        f = fi.LatticeField(sizes)
        f.add_field_constraints(w)
        f.add_points(w.data_pos, w.value_kernel, w.data_gradient if nrm is not None else 0.0, w.gradient_kernel, pd,
                     None if nrm is None else torch.from_numpy(nrm).cuda())
        return f
    f = context()
    os.environ.pop("FI_BORDER_BRUTE", None)
    wall("border prior (tree), the whole call", lambda: f.add_border_prior(0.001), REPS)
    fb = context()
    os.environ["FI_BORDER_BRUTE"] = "1"
    t0 = time.perf_counter()
    for _ in range(brute_reps(kind)):
        fb.add_border_prior(0.001)
    torch.cuda.synchronize()
    print("%-46s %10.3f ms per call (wall)" % ("border prior (FI_BORDER_BRUTE), the whole call",
                                               1e3 * (time.perf_counter() - t0) / brute_reps(kind)))
    os.environ.pop("FI_BORDER_BRUTE", None)
    ft = context()                                    # as many tree priors as brute-force ones: the same rows
    for _ in range(brute_reps(kind)):
        ft.add_border_prior(0.001)
    print("prior rows equal with and without FI_BORDER_BRUTE (Atb): %s" % np.array_equal(ft.Atb(), fb.Atb()))
    del fb, ft

    idx = fi.PointIndex(pd)
    rng = np.random.default_rng(0)
    q = (rng.uniform(0, 1, size=(NQ, 3)) * (np.array(sizes) - 1)).astype(np.float32)
    cell = np.floor(q).astype(np.int64)
    qs = q[np.argsort(cell[:, 0] + sizes[0] * (cell[:, 1] + sizes[1] * cell[:, 2]), kind="stable")]
    for label, qq in (("1 M random queries", q), ("1 M sorted queries", qs)):
        qd = torch.from_numpy(qq).cuda()
        wall(label, lambda: idx.nearest(qd, indices=True), REPS)
    for md in (float("inf"), 4.0):
        wall("distance field, max_distance = %g" % md, lambda: idx.distance_field(sizes, max_distance=md, indices=True, device=True),
             REPS)
    d = idx.distance_field(sizes, device=True)
    print("distance field: %d lattice points, max %.3f, median %.3f" % (d.numel(), float(d.max()), float(d.median())))


def summarize(path, kind):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    # the builds come first: the launches before the first kernel that is neither a build kernel (fi_bvh.h's k_bvh_*), rocPRIM's sort nor the
    # runtime's blits (the zeroed tail of a new buffer, the read-back of the finite count)
    build = []
    for _, d, k in rows:
        if not ("k_bvh_" in k or "rocprim" in k or "__amd_rocclr" in k):
            break
        build.append((d, k))
    builds = 1 + REPS
    print("| phase | launches timed | median µs | min µs |")
    print("|---|---:|---:|---:|")
    print("| build (every kernel of %d builds, summed per build) | %d launches per build | %.1f | - |"
          % (builds, len(build) // builds, sum(d for d, _ in build) / builds * 1e-3))
    used = {}
    for label, key, count in phases(kind):
        mine = [d for _, d, k in rows if key in k]
        start = used.get(key, 0)
        chunk = mine[start: start + count]
        used[key] = start + count
        timed = chunk[1:] if count > 1 else chunk
        if not timed:
            print("| %s | 0 | - | - |" % label)
            continue
        print("| %s | %d | %.1f | %.1f |" % (label, len(timed), np.median(timed) * 1e-3, np.min(timed) * 1e-3))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "summarize":
        summarize(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else "config4", int(sys.argv[2]) if len(sys.argv) > 2 else 0)
