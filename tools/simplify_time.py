"""Times fi_mesh_simplify on the device meshes of fi_iso_extract at 512^3, next to the extraction itself and to the copy to the
host that the smaller mesh saves; run it under rocprofv3 --kernel-trace --stats, in a run of its own, for the per-kernel times of
k_simp_* and the sorts (profiles/simplify.md holds the numbers).

    python tools/simplify_time.py sphere [side] [cells]    tools/iso_time.py's analytic sphere, handed in from the host
    python tools/simplify_time.py config5 [side] [cells]   config 5 (bench.py --config 5 settings) solved, its iso-surface
                                                           extracted in place
    cells: comma-separated cell edges (default 2,4,8 for the sphere, 2 for config 5)

The mesh is extracted once; every (cell, placement) is simplified once as a warm-up and 5 times timed.  Every call is
synchronous; the times are wall times around the C calls.
"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import field_interpolation_amd as fi  # noqa: E402
from field_interpolation_amd import _capi  # noqa: E402
from field_interpolation_amd import bench_settings as bs  # noqa: E402
from field_interpolation_amd import synth  # noqa: E402

REPS = 6  # the first is the warm-up


def _median(v):
    return "median of %d: %.2f ms (min %.2f, max %.2f)" % (len(v) - 1, statistics.median(v[1:]), min(v[1:]), max(v[1:]))


def _copy_ms(h):
    """wall times of fi_mesh_copy of everything to pageable host arrays"""
    L = _capi.lib()
    nv, np_ = C.c_long(0), C.c_long(0)
    _capi.check(L.fi_mesh_info(h, C.byref(nv), C.byref(np_), None))
    v, n = np.empty((nv.value, 3), np.float32), np.empty((nv.value, 3), np.float32)
    i, k = np.empty((np_.value, 3), np.int32), np.empty(nv.value, np.int64)
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        _capi.check(L.fi_mesh_copy(h, C.c_void_p(v.ctypes.data), C.c_void_p(n.ctypes.data), C.c_void_p(i.ctypes.data),
                                   C.c_void_p(k.ctypes.data), _capi.FI_HOST))
        out.append(1e3 * (time.perf_counter() - t0))
    return nv.value, np_.value, out


def run(extract, cells):
    L = _capi.lib()
    ext = []
    h = None
    for _ in range(REPS):
        if h is not None:
            L.fi_mesh_destroy(h)
        t0 = time.perf_counter()
        h = extract()
        ext.append(1e3 * (time.perf_counter() - t0))
    nv, np_, cp = _copy_ms(h)
    print("%d vertices, %d triangles" % (nv, np_))
    print("%-28s %s" % ("extract", _median(ext)))
    print("%-28s %s" % ("copy to the host", _median(cp)))
    for cell in cells:
        for placement, name in ((0, "quadric"), (1, "mean")):
            times, out = [], None
            for _ in range(REPS):
                if out is not None:
                    L.fi_mesh_destroy(out)
                out = C.c_void_p()
                t0 = time.perf_counter()
                _capi.check(L.fi_mesh_simplify(h, float(cell), None, placement, None, _capi.FI_HOST, C.byref(out)))
                times.append(1e3 * (time.perf_counter() - t0))
            ov, op, ocp = _copy_ms(out)
            L.fi_mesh_destroy(out)
            print("%-28s %s -> %d vertices, %d triangles; its copy %s" % ("cell %g %s" % (cell, name), _median(times), ov, op, _median(ocp)))
    L.fi_mesh_destroy(h)


def sphere(n, cells):
    c = (n - 1) / 2.0 + 0.3
    ax = np.arange(n, dtype=np.float32)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    f = (np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - 0.35 * n).astype(np.float32).reshape(-1)
    del x, y, z
    sz = (C.c_int * 3)(n, n, n)       # (the field is handed in from the host: "extract" includes its upload)

    def extract():
        h = C.c_void_p()
        _capi.check(_capi.lib().fi_iso_extract_field(C.c_void_p(f.ctypes.data), 3, sz, 0.0, _capi.FI_HOST, C.byref(h)))
        return h
    print("sphere %d^3" % n)
    run(extract, cells)


def config5(n, cells):
    sizes, w, pos, nrm = synth.config5(side=n, num_points=int(round(5_000_000 * (n / 512.0) ** 2)), seed=4)
    f = bs.headline_field(fi, 5, sizes, w, by_field=True)
    f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
    f.assemble()
    _x, it, rel = f.solve_cg(None, 0, bs.SETTINGS[5]["tol"])
    print("config 5 %d^3: %d iterations, relative residual %.1e" % (n, it, rel))

    def extract():
        h = C.c_void_p()
        _capi.check(_capi.lib().fi_iso_extract(f._h, None, 0.0, _capi.FI_HOST, C.byref(h)))
        return h
    run(extract, cells)


if __name__ == "__main__":
    kind = sys.argv[1] if len(sys.argv) > 1 else "sphere"
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    default = "2,4,8" if kind == "sphere" else "2"
    cells = [float(c) for c in (sys.argv[3] if len(sys.argv) > 3 else default).split(",")]
    sphere(side, cells) if kind == "sphere" else config5(side, cells)
