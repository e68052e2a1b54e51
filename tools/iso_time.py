"""Times iso-surface extraction on the device at 512^3; run it under rocprofv3 --kernel-trace --stats for the per-kernel times
of k_iso_* (profiles/iso_surface.md holds the numbers).

    python tools/iso_time.py sphere [side]    an analytic sphere field handed in from the host; the mesh is then checked
                                              for watertightness, orientation and Euler characteristic 2 on the host
    python tools/iso_time.py config5 [side]   config 5 (bench.py --config 5 settings) solved, then extracted with
                                              solution=None (in place on the device) and, for comparison, from the solution
                                              solve_cg downloaded, handed back in from the host
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import field_interpolation_amd as fi  # noqa: E402
from field_interpolation_amd import bench_settings as bs  # noqa: E402
from field_interpolation_amd import synth  # noqa: E402


def timed(what, fn):
    t0 = time.perf_counter()
    r = fn()
    print("%s: %.1f ms" % (what, 1e3 * (time.perf_counter() - t0)))
    return r


def sphere(n):
    import iso_reference as R
    c = (n - 1) / 2.0 + 0.3
    ax = np.arange(n, dtype=np.float32)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    f = (np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - 0.35 * n).astype(np.float32).reshape(-1)
    del x, y, z
    fi.iso_surface(f, [n, n, n])  # warm-up (allocations, code objects)
    m = timed("sphere %d^3: fi.iso_surface (host field in, host mesh out)" % n, lambda: fi.iso_surface(f, [n, n, n]))
    print("%d vertices, %d triangles" % (len(m.vertices), len(m.indices)))
    print("watertight and oriented: %s, Euler characteristic %d"
          % (R.watertight_oriented(m.indices), R.euler_characteristic(len(m.vertices), m.indices)))


def config5(n):
    sizes, w, pos, nrm = synth.config5(side=n, num_points=int(round(5_000_000 * (n / 512.0) ** 2)), seed=4)
    f = bs.headline_field(fi, 5, sizes, w, by_field=True)
    f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
    f.assemble()
    x, it, rel = timed("config 5 %d^3: assemble + solve_cg(out=host)" % n, lambda: f.solve_cg(None, 0, bs.SETTINGS[5]["tol"]))
    print("%d iterations, relative residual %.1e" % (it, rel))
    f.iso_surface()  # warm-up
    a = timed("iso_surface(solution=None): in place, host mesh out", lambda: f.iso_surface())
    b = timed("fi.iso_surface(downloaded solution): host field in, host mesh out", lambda: fi.iso_surface(x, sizes))
    print("%d vertices, %d triangles; identical: %s" % (len(a.vertices), len(a.indices),
                                                        all(np.array_equal(u, v) for u, v in zip(a, b))))


if __name__ == "__main__":
    kind = sys.argv[1] if len(sys.argv) > 1 else "sphere"
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    sphere(side) if kind == "sphere" else config5(side)
