"""Times the mesh-parts calls (fi_mesh_parts, fi_mesh_measure, fi_mesh_select) on the device meshes of fi_iso_extract at 512^3;
run it under rocprofv3 --kernel-trace --stats, in a run of its own, for the per-kernel times of k_parts_* and the sorts
(profiles/mesh_parts.md holds the numbers).

    python tools/parts_time.py sphere [side]    tools/iso_time.py's analytic sphere, handed in from the host
    python tools/parts_time.py config5 [side]   config 5 (bench.py --config 5 settings) solved, its iso-surface extracted in place

Each repetition extracts the mesh again: the labelling and the rows are kept with a mesh handle, so a second call on the same
handle would time a copy.  Every call is synchronous; the times are wall times around the C calls.
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


def run(extract):
    L = _capi.lib()
    times = {k: [] for k in ("extract", "parts", "measure", "select all", "select largest")}
    rows = None
    for _ in range(REPS):
        t = [time.perf_counter()]
        h = extract()
        t.append(time.perf_counter())
        count = C.c_long(0)
        _capi.check(L.fi_mesh_parts(h, C.byref(count), None, None, _capi.FI_HOST))
        t.append(time.perf_counter())
        rows = (_capi.FiMeshPart * max(count.value, 1))()
        _capi.check(L.fi_mesh_measure(h, count.value, C.cast(rows, C.c_void_p), None))
        t.append(time.perf_counter())
        keep = np.ones(count.value, np.uint8)
        out = C.c_void_p()
        _capi.check(L.fi_mesh_select(h, count.value, C.c_void_p(keep.ctypes.data), C.byref(out)))
        t.append(time.perf_counter())
        L.fi_mesh_destroy(out)
        sizes = [rows[c].size for c in range(count.value)]
        keep[:] = 0
        keep[int(np.argmax(sizes))] = 1
        t5 = time.perf_counter()
        _capi.check(L.fi_mesh_select(h, count.value, C.c_void_p(keep.ctypes.data), C.byref(out)))
        t6 = time.perf_counter()
        L.fi_mesh_destroy(out)
        nv, np_ = C.c_long(0), C.c_long(0)
        _capi.check(L.fi_mesh_info(h, C.byref(nv), C.byref(np_), None))
        L.fi_mesh_destroy(h)
        for k, d in zip(times, (t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t6 - t5)):
            times[k].append(1e3 * d)
    print("%d vertices, %d triangles, %d parts" % (nv.value, np_.value, count.value))
    order = sorted(range(count.value), key=lambda c: -rows[c].size)[:5]
    for c in order:
        r = rows[c]
        print("  part %d: %d vertices, %d triangles, %d edges, boundary %d, irregular %d, area %.6g, enclosed %.6g"
              % (c, r.vertices, r.primitives, r.edges, r.boundary, r.irregular, r.size, r.enclosed))
    for k, v in times.items():
        print("%-15s median of %d: %.2f ms (min %.2f, max %.2f)" % (k, len(v) - 1, statistics.median(v[1:]), min(v[1:]), max(v[1:])))


def sphere(n):
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
    print("sphere %d^3 (analytic: area %.6g, volume %.6g)" % (n, 4 * np.pi * (0.35 * n) ** 2, 4 / 3 * np.pi * (0.35 * n) ** 3))
    run(extract)


def config5(n):
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
    run(extract)


if __name__ == "__main__":
    kind = sys.argv[1] if len(sys.argv) > 1 else "sphere"
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    sphere(side) if kind == "sphere" else config5(side)
