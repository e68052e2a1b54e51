"""Times the k-nearest-point search and the normal estimation (fi_knn.hip) on the device; run it under rocprofv3
--kernel-trace for the per-kernel times, then summarise the trace (profiles/normals.md holds the numbers).  Queries and
outputs live on the device (torch tensors), so a call is one kernel launch and nothing else.

    python tools/normals_time.py config4 [side]   config 4's 1 M points uniformly random in its 256^3 lattice
    python tools/normals_time.py config5 [side]   config 5's 5 M points on a sphere in its 512^3 lattice
    python tools/normals_time.py summarize <kernel_trace.csv>

Every phase queries the cloud against itself, once as a warm-up and REPS times timed, in this order: nearest() (the k = 1
yardstick) over the points in input order, then over the points sorted by lattice cell (what a caller can do to make the
waves coherent; estimate_normals itself walks the tree's own sorted slots); knn at k = 8, 16, 32 in both orders;
estimate_normals at k = 16.  `summarize` splits the trace's launches of each kernel by that order and prints the medians.
"""
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5
KS = (8, 16, 32)


def phases():
    """[(label, kernel-name substring, launches)] in launch order (the first launch of each is the warm-up)"""
    out = [("nearest, input order", "k_nearest_query<3, 0>", 1 + REPS), ("nearest, sorted by cell", "k_nearest_query<3, 0>", 1 + REPS)]
    for k in KS:
        out.append(("knn k = %d, input order" % k, "k_knn_query<3, %d>" % k, 1 + REPS))
        out.append(("knn k = %d, sorted by cell" % k, "k_knn_query<3, %d>" % k, 1 + REPS))
    out.append(("estimate_normals k = 16 (sorted slots)", "k_knn_normals<3, 16>", 1 + REPS))
    return out


def points(kind, side):
    from field_interpolation_amd import synth
    if kind == "config4":
        side = side or 256
        sizes, _, pos, _ = synth.config4(side=side, num_points=int(round(1_000_000 * (side / 256.0) ** 3)), seed=3)
        return sizes, pos
    side = side or 512
    sizes, _, pos, _ = synth.config5(side=side, num_points=int(round(5_000_000 * (side / 512.0) ** 2)), seed=4)
    return sizes, pos


def wall(label, fn):
    import torch
    fn()  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    torch.cuda.synchronize()
    print("%-46s %10.3f ms per call (wall)" % (label, 1e3 * (time.perf_counter() - t0) / REPS))


def main(kind, side):
    import torch

    import field_interpolation_amd as fi
    sizes, pos = points(kind, side)
    print("%s: %d points, lattice %s" % (kind, len(pos), "x".join(map(str, sizes))))
    cell = np.floor(pos).astype(np.int64)
    by_cell = pos[np.argsort(cell[:, 0] + sizes[0] * (cell[:, 1] + sizes[1] * cell[:, 2]), kind="stable")]
    pd, ps = torch.from_numpy(pos).cuda(), torch.from_numpy(by_cell).cuda()
    idx = fi.PointIndex(pd)
    for label, q in (("input order", pd), ("sorted by cell", ps)):
        wall("nearest, " + label, lambda: idx.nearest(q, indices=True))
    for k in KS:
        for label, q in (("input order", pd), ("sorted by cell", ps)):
            wall("knn k = %d, %s" % (k, label), lambda: idx.knn(q, k))
    wall("estimate_normals k = 16", lambda: idx.estimate_normals(k=16, variation=True, device=True))
    d = idx.knn(pd, 16, indices=False)
    print("distance to the 16th neighbour: median %.3f, max %.3f" % (float(d[:, 15].median()), float(d[:, 15].max())))


def summarize(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    print("| phase | launches timed | median µs | min µs |")
    print("|---|---:|---:|---:|")
    used = {}
    for label, key, count in phases():
        mine = [d for _, d, k in rows if key in k]
        start = used.get(key, 0)
        timed = mine[start: start + count][1:]
        used[key] = start + count
        if not timed:
            print("| %s | 0 | - | - |" % label)
            continue
        print("| %s | %d | %.1f | %.1f |" % (label, len(timed), np.median(timed) * 1e-3, np.min(timed) * 1e-3))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "summarize":
        summarize(sys.argv[2])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else "config4", int(sys.argv[2]) if len(sys.argv) > 2 else 0)
