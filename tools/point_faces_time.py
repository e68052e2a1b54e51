"""Times what a call through either face of a point-set operation costs on the host (profiles/point_faces.md): single-query
fi_points_nearest and fi_nearest calls through ctypes on a set of 1000 points in 3-D, host buffers, the search structures built
before the clock starts.  CALLS calls in a loop, REPEATS times; prints the median, the fastest and the slowest repeat in
microseconds per call.  FI_HIP_LIB chooses the library, so two builds can be compared in one session.

    python tools/point_faces_time.py
"""
import ctypes as C
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS, REPEATS = 3000, 9


def main():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    L = _capi.lib()
    rng = np.random.default_rng(0)
    pos = rng.uniform(0, 31, size=(1000, 3)).astype(np.float32)
    f = fi.LatticeField([32, 32, 32])
    f.add_field_constraints(fi.Weights())
    f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, pos)
    pi = fi.PointIndex(pos)
    q = np.array([[15.5, 16.25, 14.75]], np.float32)
    d, i = np.empty(1, np.float32), np.empty(1, np.int64)
    qp, dp, ip = (C.c_void_p(a.ctypes.data) for a in (q, d, i))
    print("library: %s" % _capi.LIB_PATH)
    for name, fn, h in (("fi_points_nearest", L.fi_points_nearest, pi._h), ("fi_nearest", L.fi_nearest, f._h)):
        for _ in range(200):                                    # the structure of the context is built here
            assert fn(h, 1, qp, math.inf, dp, ip, 0) == 0
        per_call = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn(h, 1, qp, math.inf, dp, ip, 0)
            per_call.append((time.perf_counter() - t0) / CALLS * 1e6)
        print("%-18s median %.3f us per call (min %.3f, max %.3f; %d repeats of %d calls; index %d at %.4f)"
              % (name, float(np.median(per_call)), min(per_call), max(per_call), REPEATS, CALLS, i[0], d[0]))


if __name__ == "__main__":
    main()
