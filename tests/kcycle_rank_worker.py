#!/usr/bin/env python3
"""Worker of tests/test_gpu_kcycle_slabs.py, started by torch.distributed.run with 2 or 4 ranks on ONE GPU: one slab per
process with FI_OPT_MG_KCYCLE set, halo planes and dot products through the host-staged test transport (fi_comm_init_host),
like tests/two_rank_worker.py.  Every case solves to its tolerance, then counts the collectives of a fixed number of
iterations with the K-cycle and with FI_NO_KCYCLE (the V-cycle on the same slabs).  Rank 0 also solves the undivided problem
with the same settings and compares."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch
import torch.distributed as dist

dist.init_process_group("gloo")     # before any GPU call
rank, world = dist.get_rank(), dist.get_world_size()

import field_interpolation_amd as fi                      # noqa: E402
from field_interpolation_amd import bench_settings as bs  # noqa: E402
from field_interpolation_amd import dist as fdist         # noqa: E402
from field_interpolation_amd import synth                 # noqa: E402
from util import sphere_points                            # noqa: E402

torch.cuda.set_device(0)

COUNT_ITERATIONS = 5    # iterations of the collective count (fewer than 8: no wall-clock guard all-reduce among them)


def run(name, sizes, pos, nrm, dtype, tol, levels, kcycle, mixed=False, coarse_tol=None, cheb=None, by_field=False, w=None):
    w = w if w is not None else fi.Weights()

    def configure(f):
        f.add_field_constraints(w)
        bs.configure(f, levels, coarse_tol if coarse_tol else (1e-6 if dtype == "f64" else 1e-5), mixed=mixed, by_field=by_field,
                     kcycle=kcycle, cheb=cheb)

    f = fi.LatticeField(sizes, dtype=dtype, rank=rank, nranks=world)
    fdist.init_comm(f, None, host_staged=True)
    configure(f)
    zlo, zhi = f.point_range()
    z = pos[:, len(sizes) - 1]
    keep = (z >= zlo) & (z < zhi)
    f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos[keep], nrm[keep], None)
    f.assemble()
    x, it, rel = f.solve_cg(None, 0, tol)
    true_rel = f.true_residual()
    st = f.stats()
    x = np.array(x, copy=True)
    # the collectives of COUNT_ITERATIONS iterations (residual rule, unreachable tolerance: the solve runs them all), K-cycle
    # against the V-cycle on the same slabs
    f.set_field_tolerance(0.0)
    f.solve_cg(None, COUNT_ITERATIONS, 1e-30)
    red_k, it_k = f.stats()["reductions"], f.stats()["iterations"]
    os.environ["FI_NO_KCYCLE"] = "1"
    f.solve_cg(None, COUNT_ITERATIONS, 1e-30)
    red_v, it_v = f.stats()["reductions"], f.stats()["iterations"]
    del os.environ["FI_NO_KCYCLE"]
    parts = [None] * world
    dist.gather_object((x, it, rel, true_rel, int(keep.sum()), st["converged"], st["field_estimate"], st["field_rounds"], st["reductions"],
                        red_k, it_k, red_v, it_v), parts if rank == 0 else None, dst=0)
    out = None
    if rank == 0:
        xs = np.concatenate([p[0] for p in parts])
        one = fi.LatticeField(sizes, dtype=dtype)
        configure(one)
        one.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
        one.assemble()
        x1, it1, rel1 = one.solve_cg(None, 0, tol)
        x1 = np.asarray(one.solution_f64() if dtype == "f64" else x1, np.float64)
        out = {"case": name, "sizes": sizes, "levels": levels, "kcycle": kcycle, "nranks": world, "tol": tol, "by_field": by_field,
               "num_levels": f.stats()["num_levels"], "num_levels_one": one.stats()["num_levels"],
               "iterations": [p[1] for p in parts], "iterations_one": it1, "rel": [p[2] for p in parts], "true_rel": [p[3] for p in parts],
               "points_kept": [p[4] for p in parts], "points": len(pos), "converged": [p[5] for p in parts],
               "field_estimate": [p[6] for p in parts], "field_rounds": [p[7] for p in parts], "reductions": [p[8] for p in parts],
               "count_iterations": COUNT_ITERATIONS, "reductions_k": [p[9] for p in parts], "iterations_k": [p[10] for p in parts],
               "reductions_v": [p[11] for p in parts], "iterations_v": [p[12] for p in parts],
               "max_diff": float(np.abs(xs - x1).max() / np.abs(x1).max())}
        del one
    del f
    dist.barrier()
    return out


results = []
cases = os.environ.get("FI_WORKER_CASES", "pair")
if cases == "pair":
    # two slabs; 96^3 with three levels: 48^3 and 24^3 are K-levels (12^3 is the small-level engine's on the undivided lattice)
    rng = np.random.default_rng(21)
    sizes = [96, 96, 96]
    pos, nrm = sphere_points(rng, sizes, 6000)
    results.append(run("SDF 96^3, 2 slabs, K-cycle 2, f64 mixed, 3 levels", sizes, pos, nrm, "f64", 1e-8, 3, 2, mixed=True))
    rng = np.random.default_rng(22)
    sizes = [48, 40, 64]
    pos, nrm = sphere_points(rng, sizes, 3000)
    results.append(run("SDF 48x40x64, 2 slabs, K-cycle 1, f32, 2 levels", sizes, pos, nrm, "f32", 1e-5, 2, 1))
elif cases == "tail":
    # four slabs of 16 planes: 32^3 (8 planes per slab) is a K-level, 16^3 (4) a slab level the undivided lattice runs in the
    # small-level engine, 8^3 the replicated tail -- its junction sum is made once per visit of 16^3, twice per outer cycle
    rng = np.random.default_rng(9)
    sizes = [64, 64, 64]
    pos, nrm = sphere_points(rng, sizes, 4000)
    results.append(run("SDF 64^3, 4 slabs, K-cycle 3, f64 mixed, 3 levels (8^3 replicated)", sizes, pos, nrm, "f64", 1e-8, 3, 3, mixed=True))
    results.append(run("SDF 64^3, 4 slabs, K-cycle 3, f32, 3 levels (8^3 replicated)", sizes, pos, nrm, "f32", 1e-5, 3, 3))
elif cases == "config5":
    # config 5's shape at 128^3 with bench_settings' solver for it (two levels less: the same coarsest lattice as 512^3) under the
    # field rule, four slabs
    s = bs.SETTINGS[5]
    sizes, w5, pos, nrm = synth.config5(side=128, num_points=312500, seed=4)   # (the 128^3 golden's points)
    results.append(run("config 5's shape at 128^3, 4 slabs, SETTINGS[5]", sizes, pos, nrm, "f64", s["tol"], s["levels"] - 2, s["kcycle"],
                       mixed=True, coarse_tol=s["coarse_tol"], cheb=s["cheb"], by_field=True, w=w5))
elif cases == "lopsided":
    # ALL the data in rank 0's half: rank 1 holds no points and must run the same K-levels and collectives
    rng = np.random.default_rng(11)
    sizes = [32, 32, 64]
    d = rng.normal(size=(1500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = (np.array([15.5, 15.5, 10.0]) + 6.0 * d + rng.normal(scale=0.2, size=d.shape)).astype(np.float32)
    nrm = d.astype(np.float32)
    results.append(run("lopsided SDF, K-cycle 1, f64 mixed (2 levels)", sizes, pos, nrm, "f64", 1e-8, 2, 1, mixed=True))
if rank == 0:
    print("RESULTS " + json.dumps(results), flush=True)
dist.destroy_process_group()
