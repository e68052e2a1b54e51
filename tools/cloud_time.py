"""Times the point-cloud cleaning calls (fi_cloud.hip) on the device next to their yardsticks (profiles/cloud.md holds the
numbers): neighbour_distances beside estimate_normals at the same k on the same index, radius_outliers at the radius that
holds about 16 neighbours, statistical_outliers, and thin_points at the cell that holds about 4 points beside
fi_mesh_simplify (mean placement: its key, sort and place passes) on a mesh of a comparable vertex count.

    python tools/cloud_time.py config4 [side]   config 4's 1 M points uniformly random in its 256^3 lattice
    python tools/cloud_time.py config5 [side]   config 5's 5 M points on a sphere in its 512^3 lattice
    python tools/cloud_time.py mesh [side]      the yardstick alone: fi_mesh_simplify on the analytic sphere's iso-surface

Inputs and outputs are device tensors.  Every call is made once as a warm-up and REPS times between two HIP events on the
stream the library works on; the figure is the median of the REPS event times, with the fastest and the slowest beside it.
Nothing outside the tree is read."""
import ctypes as C
import os
import statistics
import sys

import numpy as np

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
    print("%-58s median of %d: %9.3f ms (min %.3f, max %.3f)" % (label, REPS, statistics.median(ms), min(ms), max(ms)))
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
    for k in (8, 16):
        timed("estimate_normals k = %d (with variation)" % k, lambda: idx.estimate_normals(k=k, variation=True, device=True))
        mean, kth, counts = timed("neighbour_distances k = %d (mean, kth, counts)" % k, lambda: idx.neighbour_distances(k, device=True))
    radius = float(kth.median())
    keep, kept = timed("radius_outliers, radius %.3f (the median 16th neighbour), 16 neighbours" % radius,
                       lambda: idx.radius_outliers(radius, 16, device=True))
    print("%-58s %d of %d kept" % ("", kept, n))
    keep, kept = timed("radius_outliers, the same radius, 2 neighbours", lambda: idx.radius_outliers(radius, 2, device=True))
    print("%-58s %d of %d kept" % ("", kept, n))
    counts = timed("radius_count of the cloud's own points, no limit", lambda: idx.radius_count(pd, radius))
    print("%-58s mean count %.2f (the point itself included)" % ("", float(counts.float().mean())))
    keep, stats = timed("statistical_outliers k = 16, std_ratio 2", lambda: idx.statistical_outliers(16, 2.0, device=True))
    print("%-58s %d of %d kept; mean %.4f, stddev %.4f" % ("", stats["kept"], n, stats["mean"], stats["stddev"]))
    # the cell that holds about 4 points: by bisection on the number of occupied cells
    lo, hi = 0.05, 64.0
    for _ in range(24):
        cell = (lo * hi) ** 0.5
        cells = len(fi.thin_points(pd, cell))
        lo, hi = (cell, hi) if n / cells < 4.0 else (lo, cell)
    for mode in ("mean", "first"):
        out = timed("thin_points %s, cell %.3f (positions only)" % (mode, cell), lambda: fi.thin_points(pd, cell, mode=mode))
    print("%-58s %d cells, %.2f points a cell" % ("", len(out), n / len(out)))
    nd = torch.nn.functional.normalize(torch.randn(n, 3, device="cuda"))
    vd = torch.randn(n, device="cuda")
    timed("thin_points mean, normals, values and all three maps", lambda: fi.thin_points(pd, cell, nd, vd, counts=True, indices=True,
                                                                                        cell_map=True))


def mesh(side):
    import torch  # noqa: F401  (the events)

    from field_interpolation_amd import _capi
    side = side or 512
    L = _capi.lib()
    c = (side - 1) / 2.0 + 0.3
    ax = np.arange(side, dtype=np.float32)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    f = (np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - 0.35 * side).astype(np.float32).reshape(-1)
    del x, y, z
    h = C.c_void_p()
    _capi.check(L.fi_iso_extract_field(C.c_void_p(f.ctypes.data), 3, (C.c_int * 3)(side, side, side), 0.0, _capi.FI_HOST, C.byref(h)))
    nv, npr = C.c_long(0), C.c_long(0)
    _capi.check(L.fi_mesh_info(h, C.byref(nv), C.byref(npr), None))
    print("sphere %d^3: %d vertices, %d triangles" % (side, nv.value, npr.value))

    def simplify(cell):
        out = C.c_void_p()
        _capi.check(L.fi_mesh_simplify(h, cell, None, 1, None, _capi.FI_HOST, C.byref(out)))
        got = C.c_long(0)
        _capi.check(L.fi_mesh_info(out, C.byref(got), None, None))
        L.fi_mesh_destroy(out)
        return got.value
    for cell in (2.0, 3.0):
        left = timed("fi_mesh_simplify, mean placement, cell %.1f" % cell, lambda: simplify(cell))
        print("%-58s %d vertices left, %.2f vertices a cluster" % ("", left, nv.value / max(left, 1)))
    L.fi_mesh_destroy(h)


if __name__ == "__main__":
    kind = sys.argv[1] if len(sys.argv) > 1 else "config4"
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    if kind == "mesh":
        mesh(side)
    else:
        cloud(kind, side)
