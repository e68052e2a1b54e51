"""Times one robust round (fi_robust.hip) at config 4's shape with the shipped solver settings; run it under rocprofv3
--kernel-trace --stats for the per-kernel times (profiles/robust.md holds the numbers).

    python tools/robust_time.py [side]          256^3, 1 M value points (bench.py --config 4), headline solver, field rule
    python tools/robust_time.py summarize <kernel_stats.csv>

Prints: the plain step (assemble_ms / solve_ms / iterations, as bench.py measures them), then for each of ROUNDS robust
rounds the host time of the reweighting step, the re-assembly, the warm-started solve and its iterations; last the loop as
fi_solve_robust runs it.  10 % of the values are shifted by +-U(1, 3) x the noise scale so that the weights have work to do.
"""
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5
KERNELS = [("residual pass", "k_point_residual"), ("median: sort", "onesweep"), ("median: sort", "radix"), ("median: pick", "k_pick_scale"),
           ("weight pass", "k_robust_weights"), ("re-emission", "k_emit_rows")]


def main(side):
    import field_interpolation_amd as fi
    from field_interpolation_amd import bench_settings, synth
    n = int(round(1_000_000 * (side / 256.0) ** 3))
    sizes, w, pos, val = synth.config4(side=side, num_points=n, seed=3)
    rng = np.random.default_rng(1)
    bad = rng.random(n) < 0.10
    val = np.where(bad, val + rng.uniform(1.0, 3.0, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0) * 5.0, val).astype(np.float32)
    f = bench_settings.headline_field(fi, 4, sizes, w, by_field=True)
    f.add_points(w.data_pos, w.value_kernel, 0.0, w.gradient_kernel, pos, None, None, val)
    for _ in range(3):                                   # (a context's first assembles still allocate)
        f.assemble()
        x, it, _ = f.solve_cg()
    st = f.stats()
    print("plain step: assemble %.3f ms, solve %.3f ms, %d iterations" % (st["assemble_ms"], st["solve_ms"], it))
    for k in range(ROUNDS):
        t0 = time.perf_counter()
        om, s = f.robust_reweight(x, loss="huber")
        t1 = time.perf_counter()
        f.assemble()
        x, it, _ = f.solve_cg(guess=x)
        st = f.stats()
        print("round %d: reweight %.3f ms (host), scale %.4f, %.1f %% of the weights below 1; assemble %.3f ms, solve %.3f ms, "
              "%d iterations" % (k + 1, 1e3 * (t1 - t0), s, 100.0 * float((om < 1).mean()), st["assemble_ms"], st["solve_ms"], it))
    f.reset_point_weights()
    t0 = time.perf_counter()
    _, _, rs = f.solve_robust(loss="huber", rounds=ROUNDS)
    print("fi_solve_robust, %d rounds: %.3f ms wall, %s" % (ROUNDS, 1e3 * (time.perf_counter() - t0), rs))


def summarize(path):
    rows = list(csv.DictReader(open(path)))
    for label, key in KERNELS:
        for r in rows:
            if key in r["Name"]:
                print("%-16s %-90s calls %6s  mean %10.1f ns  total %12s ns" % (label, r["Name"][:90], r["Calls"], float(r["AverageNs"]),
                                                                                r["TotalDurationNs"]))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "summarize":
        summarize(sys.argv[2])
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 256)
