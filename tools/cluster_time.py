"""Times the clustering calls (fi_cluster.hip) on the device next to their yardstick, the radius walk they extend
(profiles/cluster.md holds the numbers): PointIndex.cluster at min_points 1 and 8 beside radius_outliers and radius_count at
the same radius on the same index, and cluster_measure on the labels that result.

    python tools/cluster_time.py config4 [side]   config 4's 1 M points uniformly random in its 256^3 lattice
    python tools/cluster_time.py config5 [side]   config 5's 5 M points on a sphere in its 512^3 lattice
    python tools/cluster_time.py split [side]     config 4, every call once after a warm-up and nothing else: the run to put
                                                  under `rocprofv3 --kernel-trace --stats` for the kernels' shares

eps is the median distance to a point's 8th other neighbour, so that about half the points are core at min_points 8.  Inputs
and outputs are device tensors.  Every call is made once as a warm-up and REPS times between two HIP events on the stream the
library works on; the figure is the median of the REPS event times, with the fastest and the slowest beside it.  Nothing
outside the tree is read."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cloud_time import points, timed  # noqa: E402


def cloud(kind, side, split=False):
    import torch

    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    sizes, pos = points(kind, side)
    n = len(pos)
    print("%s: %d points, lattice %s" % (kind, n, "x".join(map(str, sizes))))
    pd = torch.from_numpy(pos).cuda()
    idx = fi.PointIndex(pd)
    eps = float(idx.neighbour_distances(8, device=True)[1].median())
    print("eps %.4f (the median 8th other neighbour)" % eps)
    if split:
        run = lambda label, fn: fn()  # noqa: E731
        idx.cluster(eps, 8, device=True)                      # warm-up: the allocations
        torch.cuda.synchronize()
    else:
        run = timed
    for least in (1, 8):
        labels, core, stats = run("cluster eps %.3f, min_points %d (labels, core, stats)" % (eps, least),
                                  lambda: idx.cluster(eps, least, core=True, stats=True, device=True))
        print("%-58s %s" % ("", stats))
        only = run("cluster, the same, labels alone", lambda: idx.cluster(eps, least, device=True))
        assert torch.equal(only, labels)
        rows = run("cluster_measure of these labels, %d clusters" % stats["clusters"],
                   lambda: fi.cluster_measure(pd, labels, core, num_clusters=stats["clusters"]))
        print("%-58s largest cluster %d points" % ("", max([r["count"] for r in rows] + [0])))
        table = (_capi.FiClusterRow * max(stats["clusters"], 1))()   # the C call alone: no list of dicts on the host
        flags = core.to(torch.uint8)
        run("fi_cluster_measure, the same (the C call alone)",
            lambda: _capi.check(_capi.lib().fi_cluster_measure(3, n, C.c_void_p(pd.data_ptr()), C.c_void_p(labels.data_ptr()),
                                                               C.c_void_p(flags.data_ptr()), stats["clusters"], table, _capi.FI_DEVICE)))
        others = max(least - 1, 1)
        keep, kept = run("radius_outliers, the same radius, %d other neighbours" % others,
                         lambda: idx.radius_outliers(eps, others, device=True))
        print("%-58s %d of %d kept" % ("", kept, n))
    counts = run("radius_count of the cloud's own points, no limit", lambda: idx.radius_count(pd, eps))
    print("%-58s mean count %.2f (the point itself included)" % ("", float(counts.float().mean())))


if __name__ == "__main__":
    kind = sys.argv[1] if len(sys.argv) > 1 else "config4"
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    cloud("config4" if kind == "split" else kind, side, split=kind == "split")
