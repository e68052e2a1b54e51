"""Times redistancing on the device (fi_redistance*: the mesh, the surface's search structure, the signed lattice queries)
for both methods at max_distance = 4 and inf; run it under rocprofv3 --kernel-trace --stats for the per-kernel times
(profiles/redistance.md holds the numbers).

    python tools/surface_time.py sphere [side]    an analytic sphere's exact signed distance (default 512^3) from the host
    python tools/surface_time.py config5 [side]   config 5 (bench.py --config 5 settings) solved, redistanced in place
    python tools/surface_time.py config3 [side]   config 3 (default 4096^2) solved, redistanced in place
    python tools/surface_time.py summarize <kernel_trace.csv>

Each (method, max_distance) runs once to warm up and REPS times timed, in the order of COMBOS; `summarize` splits the
trace's launches into those calls (one k_bvh_bounds launch per build: fi_bvh.h's build kernels are k_bvh_*) and prints per-call medians of the build
(every build kernel, rocPRIM's sort between them included, summed) and of the signed lattice query kernel.
"""
import csv
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 3
COMBOS = [("iso", 4.0), ("iso", math.inf), ("dual", 4.0), ("dual", math.inf)]


def run(what, call):
    for method, md in COMBOS:
        call(method, md)  # warm-up (allocations, code objects)
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            d = call(method, md)
            ts.append(1e3 * (time.perf_counter() - t0))
        fin = np.isfinite(d)
        print("%s, %s, max_distance %g: %.1f ms per call (median of %d, host wall, the mesh included); %d of %d finite"
              % (what, method, md, np.median(ts), REPS, fin.sum(), d.size))


def sphere(n):
    import field_interpolation_amd as fi
    c, r = (n - 1) / 2.0 + 0.3, 0.35 * n
    ax = np.arange(n, dtype=np.float32)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    f = (np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - r).astype(np.float32).reshape(-1)
    del x, y, z
    sizes = [n, n, n]
    run("sphere %d^3 (host field in, host distances out)" % n, lambda m, md: fi.redistance(f, sizes, 0.0, m, md))


def solved(config, sizes, w, pos, nrm, by_field, levels_less=0):
    import field_interpolation_amd as fi
    from field_interpolation_amd import bench_settings as bs
    f = fi.LatticeField(sizes, dtype="f64")
    f.add_field_constraints(w)
    s = bs.SETTINGS[config]
    bs.configure(f, s["levels"] - levels_less, s["coarse_tol"], by_field=by_field, kcycle=s.get("kcycle", 0), cheb=s.get("cheb"))
    f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
    f.assemble()
    _, it, rel = f.solve_cg(None, 0, s["tol"])
    print("config %d %s: %d iterations, relative residual %.1e" % (config, "x".join(map(str, sizes)), it, rel))
    run("config %d in place" % config, lambda m, md: f.redistance(None, 0.0, m, md))


def config5(n):
    from field_interpolation_amd import synth
    sizes, w, pos, nrm = synth.config5(side=n, num_points=int(round(5_000_000 * (n / 512.0) ** 2)), seed=4)
    solved(5, sizes, w, pos, nrm, True)


def config3(n):
    from field_interpolation_amd import synth
    sizes, w, pos, nrm = synth.config3(side=n)
    solved(3, sizes, w, pos, nrm, False, int(round(np.log2(4096 / n))))  # the same coarsest lattice as at 4096


def summarize(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    # a call: from its k_bvh_bounds (the first build kernel) to the end of its query kernel
    calls, cur = [], None
    for s, e, k in rows:
        if "k_bvh_bounds" in k and "total" not in k:
            cur = {"start": s, "build": 0, "query": 0, "query_start": None}
            calls.append(cur)
        if cur is None:
            continue
        if "k_surf_query" in k:
            cur["query"] += e - s
            cur["query_start"] = s if cur["query_start"] is None else cur["query_start"]
        elif cur["query_start"] is None and ("k_bvh_" in k or "rocprim" in k):
            cur["build"] += e - s
    per = 1 + REPS
    assert len(calls) == per * len(COMBOS), (len(calls), per * len(COMBOS))
    print("| method | max_distance | build: kernels, ms (median) | build: first kernel to the query, ms | query kernel, ms (median) |")
    print("|---|---:|---:|---:|---:|")
    for i, (method, md) in enumerate(COMBOS):
        timed = calls[i * per + 1: (i + 1) * per]
        print("| %s | %g | %.3f | %.3f | %.3f |" % (method, md, np.median([c["build"] for c in timed]) * 1e-6,
                                                   np.median([c["query_start"] - c["start"] for c in timed]) * 1e-6,
                                                   np.median([c["query"] for c in timed]) * 1e-6))


if __name__ == "__main__":
    kind = sys.argv[1] if len(sys.argv) > 1 else "sphere"
    if kind == "summarize":
        summarize(sys.argv[2])
        sys.exit(0)
    side = int(sys.argv[2]) if len(sys.argv) > 2 else (4096 if kind == "config3" else 512)
    {"sphere": sphere, "config5": config5, "config3": config3}[kind](side)
