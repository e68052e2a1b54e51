"""Times the moving-least-squares projection (fi_mls.hip) on the device next to its yardsticks (profiles/mls.md is where the
numbers go): PointIndex.smooth of a cloud's own points at degree 1 and 2 and k = 8 / 16 / 32 beside estimate_normals and
neighbour_distances at the same k on the same index -- the same walk with a lighter epilogue and no scratch -- and
PointIndex.project of as many random queries.

    python tools/mls_time.py config4 [side]   config 4's 1 M points uniformly random in its 256^3 lattice
    python tools/mls_time.py config5 [side]   config 5's 5 M points on a sphere in its 512^3 lattice

The radius is the median distance to a point's k-th other neighbour, so that about half the lists are full.  Inputs and
outputs are device tensors.  Every call is made once as a warm-up and REPS times between two HIP events on the stream the
library works on; the figure is the median of the REPS event times, with the fastest and the slowest beside it.  Nothing
outside the tree is read."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5


def timed(label, fn):
    import torch
    fn()  # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    print("%-66s median of %d: %9.3f ms (min %.3f, max %.3f)" % (label, REPS, statistics.median(ms), min(ms), max(ms)))
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


def cloud(kind, side):
    import torch

    import field_interpolation_amd as fi
    sizes, pos = points(kind, side)
    n = len(pos)
    print("%s: %d points, lattice %s" % (kind, n, "x".join(map(str, sizes))))
    pd = torch.from_numpy(pos).cuda()
    idx = fi.PointIndex(pd)
    lo = torch.tensor([0.0] * len(sizes), device="cuda")
    hi = torch.tensor([float(s - 1) for s in sizes], device="cuda")
    qd = lo + (hi - lo) * torch.rand((n, len(sizes)), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    for k in (8, 16, 32):
        timed("estimate_normals k = %d (with variation)" % k, lambda: idx.estimate_normals(k=k, variation=True, device=True))
        _, kth, _ = timed("neighbour_distances k = %d (mean, kth, counts)" % k, lambda: idx.neighbour_distances(k, device=True))
        radius = float(kth[torch.isfinite(kth)].median())
        for degree in (1, 2):
            out = timed("smooth k = %d, radius %.3f, degree %d (all four outputs)" % (k, radius, degree),
                        lambda: idx.smooth(k=k, radius=radius, degree=degree, curvature=True, order=True, device=True))
            counts = torch.bincount(out[3].long(), minlength=3).tolist()
            print("%-66s order 0 / 1 / 2: %d / %d / %d" % ("", counts[0], counts[1], counts[2]))
        timed("smooth k = %d, degree 2, positions and normals only" % k, lambda: idx.smooth(k=k, radius=radius, device=True))
        out = timed("project %d random queries, k = %d, degree 2" % (n, k),
                    lambda: idx.project(qd, k=k, radius=radius, curvature=True, order=True))
        counts = torch.bincount(out[3].long(), minlength=3).tolist()
        print("%-66s order 0 / 1 / 2: %d / %d / %d" % ("", counts[0], counts[1], counts[2]))


if __name__ == "__main__":
    cloud(sys.argv[1] if len(sys.argv) > 1 else "config4", int(sys.argv[2]) if len(sys.argv) > 2 else 0)
