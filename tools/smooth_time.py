"""Times fi_mesh_smooth and fi_mesh_normals on the device mesh of fi_iso_extract at 512^3, next to the extraction itself; run it
under rocprofv3 --kernel-trace --stats, in a run of its own, for the per-kernel times of k_smooth_* and the sorts, and under
rocprofv3 --pmc (again a run of its own) for the bytes the step kernel moves (profiles/smooth.md holds the numbers).

    python tools/smooth_time.py sphere [side] [iterations]    tools/iso_time.py's analytic sphere, handed in from the host
    python tools/smooth_time.py steps [side] [iterations]     only the Taubin call (for the counter run)

The mesh is extracted once; every variant is called once as a warm-up and 5 times timed.  Every call is synchronous; the times
are wall times around the C calls.  The variants split a call: iterations = 0 with the normals kept is the check and the
copies alone, iterations = 0 with the normals recomputed adds the normals, 1 and `iterations` iterations with the normals kept
add the rows (the adjacency build) and the steps -- the difference of the last two over the steps between them is one step.
"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from field_interpolation_amd import _capi  # noqa: E402

REPS = 6  # the first is the warm-up
FIXED, SLIDE, FREE = 0, 1, 2
RECOMPUTE, KEEP = 0, 1


def _median(v):
    return "median of %d: %.3f ms (min %.3f, max %.3f)" % (len(v) - 1, statistics.median(v[1:]), min(v[1:]), max(v[1:]))


def _timed(call):
    L = _capi.lib()
    times, out = [], None
    for _ in range(REPS):
        if out is not None:
            L.fi_mesh_destroy(out)
        out = C.c_void_p()
        t0 = time.perf_counter()
        _capi.check(call(C.byref(out)))
        times.append(1e3 * (time.perf_counter() - t0))
    L.fi_mesh_destroy(out)
    return times


def _smooth(h, iterations, lam=0.5, mu=-0.53, boundary=FIXED, max_move=0.0, normals=KEEP):
    opt = _capi.FiSmoothOptions(iterations, lam, mu, boundary, max_move, normals)
    return _timed(lambda out: _capi.lib().fi_mesh_smooth(h, C.byref(opt), out))


def _algorithmic_bytes(h):
    """(vertices, triangles, entries of the rows) and the bytes one step has to move: per vertex its row (4 bytes an entry and
    its offset), |N| + 1 fp64 positions read and one written"""
    L = _capi.lib()
    nv, np_ = C.c_long(0), C.c_long(0)
    _capi.check(L.fi_mesh_info(h, C.byref(nv), C.byref(np_), None))
    idx = np.empty((np_.value, 3), np.int32)
    _capi.check(L.fi_mesh_copy(h, None, None, C.c_void_p(idx.ctypes.data), None, _capi.FI_HOST))
    t = idx.astype(np.int64)
    he = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    entries = len(np.unique(np.concatenate([he[:, 0] * nv.value + he[:, 1], he[:, 1] * nv.value + he[:, 0]])))
    return nv.value, np_.value, entries, 4 * entries + 4 * nv.value + 24 * (entries + nv.value) + 24 * nv.value


def run(extract, iterations, only_steps):
    L = _capi.lib()
    h = extract()
    if only_steps:
        print("%-44s %s" % ("%d iterations, Taubin, normals kept" % iterations, _median(_smooth(h, iterations))))
        L.fi_mesh_destroy(h)
        return
    ext = []
    for _ in range(REPS):
        L.fi_mesh_destroy(h)
        t0 = time.perf_counter()
        h = extract()
        ext.append(1e3 * (time.perf_counter() - t0))
    nv, np_, entries, step_bytes = _algorithmic_bytes(h)
    print("%d vertices, %d triangles, %d row entries (%.2f a vertex); one step moves %.1f MB algorithmically"
          % (nv, np_, entries, entries / nv, step_bytes / 1e6))
    print("%-44s %s" % ("extract", _median(ext)))
    rows = [("0 iterations, normals kept (check, copies)", _smooth(h, 0)),
            ("0 iterations, normals recomputed", _smooth(h, 0, normals=RECOMPUTE)),
            ("fi_mesh_normals", _timed(lambda out: L.fi_mesh_normals(h, out))),
            ("1 iteration, Taubin, normals kept", _smooth(h, 1)),
            ("%d iterations, Taubin, normals kept" % iterations, _smooth(h, iterations)),
            ("%d iterations, Laplacian, normals kept" % iterations, _smooth(h, iterations, mu=0.0)),
            ("%d iterations, Taubin, slide" % iterations, _smooth(h, iterations, boundary=SLIDE)),
            ("%d iterations, Taubin, free" % iterations, _smooth(h, iterations, boundary=FREE)),
            ("%d iterations, Taubin, max_move 0.5" % iterations, _smooth(h, iterations, max_move=0.5)),
            ("%d iterations, Taubin, normals recomputed" % iterations, _smooth(h, iterations, normals=RECOMPUTE))]
    for name, times in rows:
        print("%-44s %s" % (name, _median(times)))
    one, many = statistics.median(rows[3][1][1:]), statistics.median(rows[4][1][1:])
    if iterations > 1:
        step = (many - one) / (2.0 * (iterations - 1))
        print("one step: %.1f us, %.0f GB/s of algorithmic bytes; rows (the adjacency build): %.3f ms"
              % (1e3 * step, step_bytes / (1e6 * step), one - 2.0 * step - statistics.median(rows[0][1][1:])))
    L.fi_mesh_destroy(h)


def sphere(n, iterations, only_steps):
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
    run(extract, iterations, only_steps)


if __name__ == "__main__":
    kind = sys.argv[1] if len(sys.argv) > 1 else "sphere"
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    iterations = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    sphere(side, iterations, kind == "steps")
