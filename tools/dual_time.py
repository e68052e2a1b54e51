"""Times dual contouring on the device beside iso extraction on the same fields; run it under rocprofv3 --kernel-trace --stats
for the per-kernel times of k_dc_* and k_iso_* (profiles/dual_contour.md holds the numbers).

    python tools/dual_time.py sphere [side]    an analytic sphere field (default 512^3) handed in from the host; the dual
                                               mesh is then checked for closedness and volume on the host
    python tools/dual_time.py config5 [side]   config 5 (bench.py --config 5 settings) solved, then contoured in place
                                               (solution=None)
    python tools/dual_time.py config3 [side]   config 3 (default 4096^2) solved, then contoured in place
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


def both(what, dual, iso, reps=3):
    dual()
    iso()  # warm-up (allocations, code objects)
    for _ in range(reps):
        a = timed("%s: dual_contour" % what, dual)
        b = timed("%s: iso_surface" % what, iso)
    print("dual: %d vertices, %d primitives; iso: %d vertices, %d primitives"
          % (len(a.vertices), len(a.indices), len(b.vertices), len(b.indices)))
    return a, b


def sphere(n):
    from test_dual_reference import closed_oriented, signed_volume
    c, r = (n - 1) / 2.0 + 0.3, 0.35 * n
    ax = np.arange(n, dtype=np.float32)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    f = (np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - r).astype(np.float32).reshape(-1)
    del x, y, z
    sizes = [n, n, n]
    a, _ = both("sphere %d^3 (host field in, host mesh out)" % n, lambda: fi.dual_contour(f, sizes), lambda: fi.iso_surface(f, sizes))
    vol = signed_volume(a.vertices, a.indices)
    print("closed and oriented: %s; volume / (4/3 pi r^3) = %.5f" % (closed_oriented(a.indices), vol / (4.0 / 3.0 * np.pi * r ** 3)))


def solved(config, sizes, w, pos, nrm, by_field, levels_less=0):
    f = fi.LatticeField(sizes, dtype="f64")
    f.add_field_constraints(w)
    s = bs.SETTINGS[config]
    bs.configure(f, s["levels"] - levels_less, s["coarse_tol"], by_field=by_field, kcycle=s.get("kcycle", 0), cheb=s.get("cheb"))
    f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
    f.assemble()
    _, it, rel = timed("config %d %s: solve_cg" % (config, "x".join(map(str, sizes))), lambda: f.solve_cg(None, 0, bs.SETTINGS[config]["tol"]))
    print("%d iterations, relative residual %.1e" % (it, rel))
    both("in place", lambda: f.dual_contour(), lambda: f.iso_surface())


def config5(n):
    sizes, w, pos, nrm = synth.config5(side=n, num_points=int(round(5_000_000 * (n / 512.0) ** 2)), seed=4)
    solved(5, sizes, w, pos, nrm, True)


def config3(n):
    sizes, w, pos, nrm = synth.config3(side=n)
    solved(3, sizes, w, pos, nrm, False, int(round(np.log2(4096 / n))))  # the same coarsest lattice as at 4096


if __name__ == "__main__":
    kind = sys.argv[1] if len(sys.argv) > 1 else "sphere"
    side = int(sys.argv[2]) if len(sys.argv) > 2 else (4096 if kind == "config3" else 512)
    {"sphere": sphere, "config5": config5, "config3": config3}[kind](side)
