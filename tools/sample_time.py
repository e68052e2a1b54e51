"""Times point queries (fi_sample) on the device; run it under rocprofv3 --kernel-trace --stats for the per-kernel times of
k_sample* (profiles/sample.md holds the numbers).  Positions and outputs live on the device (torch tensors), so a call is the
kernel and nothing else.

    python tools/sample_time.py config4 [side]   config 4 (bench.py --config 4 settings, fp64) solved, its 1 M data points
                                                 sampled in the fp64 solution in place
    python tools/sample_time.py config5 [side]   config 5 solved (fp64), its 5 M data points sampled in place, and in the fp32
                                                 solution handed back as a device tensor (a 512 MB field at 512^3)

Every combination of linear / cubic and with / without gradients runs on the points in three orders: as generated
(uniformly random), sorted by cell on the host, and coherent along x (consecutive points step along x through the
lattice, the same count).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import field_interpolation_amd as fi  # noqa: E402
from field_interpolation_amd import bench_settings as bs  # noqa: E402
from field_interpolation_amd import synth  # noqa: E402

REPS = 20


def orders(pos, sizes):
    """{name: positions (n, 3) float32}"""
    n = len(pos)
    c = np.minimum(np.floor(pos).astype(np.int64), np.array(sizes) - 2)
    key = c[:, 0] + sizes[0] * (c[:, 1] + sizes[1] * c[:, 2])
    rng = np.random.default_rng(0)
    k = np.arange(n)
    rows = k // (sizes[0] - 1)
    line = rng.permutation(max(1, (sizes[1] - 1) * (sizes[2] - 1)))[rows % max(1, (sizes[1] - 1) * (sizes[2] - 1))]
    coherent = np.stack([(k % (sizes[0] - 1)) + 0.37, (line % (sizes[1] - 1)) + 0.61, (line // (sizes[1] - 1)) + 0.23], axis=1)
    return {"random": pos, "sorted": pos[np.argsort(key, kind="stable")], "x-coherent": coherent.astype(np.float32)}


def run(label, fn, pos, n):
    p = torch.from_numpy(np.ascontiguousarray(pos, np.float32)).cuda()
    for cubic in (False, True):
        for grads in (False, True):
            fn(p, grads, cubic)  # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                fn(p, grads, cubic)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / REPS
            print("%-34s %-6s %-5s %8.3f ms per call  %7.2f G points/s"
                  % (label, "cubic" if cubic else "linear", "grad" if grads else "-", ms, n / ms * 1e-6))


def solve(config, sizes, w, pos, nrm, val):
    f = bs.headline_field(fi, config, sizes, w, by_field=True)
    f.add_points(w.data_pos, w.value_kernel, w.data_gradient if nrm is not None else 0.0, w.gradient_kernel, pos, nrm, None,
                 values=val)
    f.assemble()
    t0 = time.perf_counter()
    x, it, rel = f.solve_cg(None, 0, bs.SETTINGS[config]["tol"])
    print("config %d %s: solved in %d iterations, %.2f s" % (config, "x".join(map(str, sizes)), it, time.perf_counter() - t0))
    return f, x


def main(kind, side):
    if kind == "config4":
        side = side or 256
        sizes, w, pos, val = synth.config4(side=side, num_points=int(round(1_000_000 * (side / 256.0) ** 3)), seed=3)
        f, x = solve(4, sizes, w, pos, None, val)
        fields = [("fp64 solution in place", lambda p, g, c: f.sample(p, gradients=g, cubic=c))]
    else:
        side = side or 512
        sizes, w, pos, nrm = synth.config5(side=side, num_points=int(round(5_000_000 * (side / 512.0) ** 2)), seed=4)
        f, x = solve(5, sizes, w, pos, nrm, None)
        xd = torch.from_numpy(x).cuda()
        fields = [("fp64 solution in place", lambda p, g, c: f.sample(p, gradients=g, cubic=c)),
                  ("fp32 field on the device", lambda p, g, c: fi.sample_field(xd, sizes, p, gradients=g, cubic=c))]
    n = len(pos)
    print("%d points, lattice %s" % (n, "x".join(map(str, sizes))))
    for oname, op in orders(np.asarray(pos, np.float32), sizes).items():
        for fname, fn in fields:
            run("%s, %s" % (fname, oname), fn, op, n)
    # a check of the device path against the host path on a few points
    q = np.asarray(pos[:1000], np.float32)
    a = f.sample(q)
    b = f.sample(torch.from_numpy(q).cuda()).cpu().numpy()
    print("device and host positions agree: %s" % np.array_equal(a.view(np.uint32), b.view(np.uint32)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "config4", int(sys.argv[2]) if len(sys.argv) > 2 else 0)
