"""Times fi_mesh_sample and fi_mesh_deviation on the device mesh of fi_iso_extract at 512^3 against its simplification, next to
the walk they feed: fi_surface_distance on the same staged points.  Run it under rocprofv3 --kernel-trace --stats, in a run
of its own, for the per-kernel times of k_mpts_* (profiles/meshpts.md holds the numbers).

    python tools/meshpts_time.py sphere [side] [samples] [cell]    tools/iso_time.py's analytic sphere, handed in from the host

The mesh is extracted and simplified once (cell 4 at 512^3: 35 k vertices); every call is made once as a warm-up and 5 times
timed.  Every call is synchronous; the times are wall times around the C calls, outputs in device memory.  The rows split a
deviation call: sampling alone, the walk alone on the sampler's points (tools/surface_time.py's method: the host clock around
fi_surface_distance), then the whole call -- what it adds to the walks of its two lists is sampling, staging and reduction."""
import ctypes as C
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from field_interpolation_amd import _capi  # noqa: E402

REPS = 6  # the first is the warm-up
FACE, VERTEX = 0, 1


def _median(v):
    return "median of %d: %.3f ms (min %.3f, max %.3f)" % (len(v) - 1, statistics.median(v[1:]), min(v[1:]), max(v[1:]))


def _timed(call):
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        _capi.check(call())
        times.append(1e3 * (time.perf_counter() - t0))
    return times


class Device:
    """device buffers of the process's HIP runtime (the one libfi_hip.so is linked against)"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.held = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 16))) == 0
        self.held.append(p)
        return p

    def release(self):
        for p in self.held:
            self.hip.hipFree(p)
        self.held = []


def run(extract, samples, cell):
    L = _capi.lib()
    dev = Device()
    fine = extract()
    coarse = C.c_void_p()
    _capi.check(L.fi_mesh_simplify(fine, cell, None, 0, None, _capi.FI_HOST, C.byref(coarse)))
    sizes = []
    for h in (fine, coarse):
        nv, np_ = C.c_long(0), C.c_long(0)
        _capi.check(L.fi_mesh_info(h, C.byref(nv), C.byref(np_), None))
        sizes.append((nv.value, np_.value))
    print("the mesh: %d vertices, %d triangles; simplified at cell %g: %d vertices, %d triangles" % (sizes[0] + (cell,) + sizes[1]))
    s_fine, s_coarse = C.c_void_p(), C.c_void_p()
    _capi.check(L.fi_surface_from_mesh(C.byref(s_fine), fine))
    _capi.check(L.fi_surface_from_mesh(C.byref(s_coarse), coarse))
    pos, nrm, prim = dev.alloc(12 * samples), dev.alloc(12 * samples), dev.alloc(8 * samples)
    pos_coarse = dev.alloc(12 * samples)   # (a buffer of its own: `pos` keeps the mesh's samples for the walk below)
    dist = dev.alloc(4 * max(samples, sizes[0][0]))
    vd = dev.alloc(4 * sizes[0][0])
    of_s, of_v = _capi.FiDeviation(), _capi.FiDeviation()
    D = _capi.FI_DEVICE
    inf = math.inf

    def deviation(a, b, n, structs=True, distances=None):
        return L.fi_mesh_deviation(a, b, n, 1, inf, C.byref(of_s) if structs else None, C.byref(of_v), distances, D)

    rows = [("fi_mesh_sample, positions only", lambda: L.fi_mesh_sample(fine, samples, 1, FACE, pos, None, None, D)),
            ("fi_mesh_sample, face normals, primitives", lambda: L.fi_mesh_sample(fine, samples, 1, FACE, pos, nrm, prim, D)),
            ("fi_mesh_sample, vertex normals, primitives", lambda: L.fi_mesh_sample(fine, samples, 1, VERTEX, pos, nrm, prim, D)),
            ("fi_mesh_sample of the simplified mesh", lambda: L.fi_mesh_sample(coarse, samples, 1, FACE, pos_coarse, None, None, D)),
            ("fi_surface_distance, the samples -> simplified", None),
            ("fi_mesh_deviation -> simplified, samples + vertices", lambda: deviation(fine, s_coarse, samples)),
            ("fi_mesh_deviation -> simplified, vertices only", lambda: deviation(fine, s_coarse, 0, False)),
            ("fi_mesh_deviation -> simplified, + vertex_distances", lambda: deviation(fine, s_coarse, samples, True, vd)),
            ("fi_mesh_deviation simplified -> the mesh", lambda: deviation(coarse, s_fine, samples))]
    # the walk alone: on the mesh's samples, which rows 0 to 2 leave in `pos` (the same points every time: seed 1)
    rows[4] = (rows[4][0], lambda: L.fi_surface_distance(s_coarse, samples, pos, inf, dist, None, None, D))
    for name, call in rows:
        if "deviation" in name:
            C.memset(C.byref(of_s), 0, C.sizeof(of_s))   # (a call that is not given the struct leaves zeros to print)
        print("%-52s %s" % (name, _median(_timed(call))))
        if "deviation" in name:
            print("%-52s samples (%d): max %.4g mean %.4g rms %.4g;  vertices (%d): max %.4g mean %.4g rms %.4g"
                  % ("", of_s.queries, of_s.max, of_s.mean, of_s.rms, of_v.queries, of_v.max, of_v.mean, of_v.rms))
    for h in (s_fine, s_coarse):
        L.fi_surface_destroy(h)
    for h in (fine, coarse):
        L.fi_mesh_destroy(h)
    dev.release()


def sphere(n, samples, cell):
    c = (n - 1) / 2.0 + 0.3
    ax = np.arange(n, dtype=np.float32)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    f = (np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - 0.35 * n).astype(np.float32).reshape(-1)
    del x, y, z
    sz = (C.c_int * 3)(n, n, n)

    def extract():
        h = C.c_void_p()
        _capi.check(_capi.lib().fi_iso_extract_field(C.c_void_p(f.ctypes.data), 3, sz, 0.0, _capi.FI_HOST, C.byref(h)))
        return h
    print("sphere %d^3, %d samples" % (n, samples))
    run(extract, samples, cell)


if __name__ == "__main__":
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    samples = int(sys.argv[3]) if len(sys.argv) > 3 else 1000000
    cell = float(sys.argv[4]) if len(sys.argv) > 4 else 4.0
    sphere(side, samples, cell)
