"""Times fi_mesh_register on the device mesh of fi_iso_extract at 512^3, next to the walk it drives: fi_surface_distance on the
same staged points.  Run it under rocprofv3 --kernel-trace --stats, in a run of its own, for the per-kernel times of k_reg_*
and of the walk (profiles/register.md holds the numbers).

    python tools/register_time.py sphere [side] [points] [steps]    tools/iso_time.py's analytic sphere, handed in from the host

The mesh is extracted once and its search structure built once; `points` sample_mesh points of it (seed 1) are turned by one
degree about (1, 2, 3), shifted by (0.3, -0.2, 0.25) and staged on the device.  Every call is made once as a warm-up and 5
times timed.  Every call is synchronous; the times are wall times around the C calls, everything in device memory.  The rows:
the walk alone (distances only; with primitives and closest points, as the unit asks for them), one evaluation
(max_iterations = 0) and `steps` steps with tolerances of 0, which never stop early: steps + 1 evaluations, so that
(the second - the first) / steps is what a step of the loop costs and the first minus the walk what the unit adds to it."""
import ctypes as C
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from field_interpolation_amd import _capi  # noqa: E402

REPS = 6  # the first is the warm-up


def _timed(call):
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        _capi.check(call())
        times.append(1e3 * (time.perf_counter() - t0))
    return times


def _row(name, v):
    print("%-58s median of %d: %.3f ms (min %.3f, max %.3f)" % (name, len(v) - 1, statistics.median(v[1:]), min(v[1:]), max(v[1:])))
    return statistics.median(v[1:])


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

    def download(self, p, array):
        assert self.hip.hipMemcpy(C.c_void_p(array.ctypes.data), p, C.c_size_t(array.nbytes), 2) == 0

    def upload(self, p, array):
        assert self.hip.hipMemcpy(p, C.c_void_p(array.ctypes.data), C.c_size_t(array.nbytes), 1) == 0

    def release(self):
        for p in self.held:
            self.hip.hipFree(p)
        self.held = []


def run(extract, points, steps):
    import register_reference as G
    L = _capi.lib()
    dev = Device()
    mesh = extract()
    nv, np_ = C.c_long(0), C.c_long(0)
    _capi.check(L.fi_mesh_info(mesh, C.byref(nv), C.byref(np_), None))
    print("the mesh: %d vertices, %d triangles" % (nv.value, np_.value))
    surface = C.c_void_p()
    _capi.check(L.fi_surface_from_mesh(C.byref(surface), mesh))
    D = _capi.FI_DEVICE
    pos, moved, dist = dev.alloc(12 * points), dev.alloc(12 * points), dev.alloc(4 * points)
    prim, closest = dev.alloc(8 * points), dev.alloc(12 * points)
    _capi.check(L.fi_mesh_sample(mesh, points, 1, 0, pos, None, None, D))
    on = np.empty((points, 3), np.float32)
    dev.download(pos, on)
    Rs, shift = G.rotation((1, 2, 3), 1.0), (0.3, -0.2, 0.25)
    dev.upload(pos, G.moved(on, Rs, shift))
    R, t = G.truth(on, Rs, shift)
    res = _capi.FiRegistration()
    inf = math.inf

    def register(mode, iterations, index=surface):
        opt = _capi.FiRegisterOptions(mode, iterations, inf, 0.0, 0.0, _capi.FI_LOSS_NONE, 0.0, 0.0)
        return lambda: L.fi_mesh_register(mesh, index, points, pos, C.byref(opt), None, C.byref(res), moved, dist, D)

    _row("fi_surface_distance, distances only", _timed(lambda: L.fi_surface_distance(surface, points, pos, inf, dist, None, None, D)))
    full = _row("fi_surface_distance, + primitives and closest points",
                _timed(lambda: L.fi_surface_distance(surface, points, pos, inf, dist, prim, closest, D)))
    for mode, name in ((0, "plane"), (1, "point")):
        one = _row("fi_mesh_register %s, max_iterations 0 (one evaluation)" % name, _timed(register(mode, 0)))
        many = _row("fi_mesh_register %s, %d steps (%d evaluations)" % (name, steps, steps + 1), _timed(register(mode, steps)))
        T = np.array(list(res.transform)).reshape(4, 4)
        print("%-58s one evaluation adds %.3f ms to the walk it drives (%.3f ms); a step of the loop costs %.3f ms; rotation off by %.2g,"
              " translation by %.2g, rms %.3g, fixed_mask %d" % ("", one - full, full, (many - one) / steps, np.abs(T[:3, :3] - R).max(),
                                                                 np.abs(T[:3, 3] - t).max(), res.rms, res.fixed_mask))
    _row("fi_mesh_register plane, one evaluation, index built for the call", _timed(register(0, 0, None)))
    L.fi_surface_destroy(surface)
    L.fi_mesh_destroy(mesh)
    dev.release()


def sphere(n, points, steps):
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
    print("sphere %d^3, %d points, %d steps" % (n, points, steps))
    run(extract, points, steps)


if __name__ == "__main__":
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    points = int(sys.argv[3]) if len(sys.argv) > 3 else 1000000
    steps = int(sys.argv[4]) if len(sys.argv) > 4 else 4
    sphere(side, points, steps)
