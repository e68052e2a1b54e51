"""FI_OPT_MG_KCYCLE over slabs: a decomposed lattice -- a loop-back group (all slabs in one process) or one slab per process
(the host-staged test transport, tests/kcycle_rank_worker.py) -- runs the undivided lattice's K-cycle: the same K-levels, two
flexible-CG steps per K-level visit whose dot products are summed over the slabs in one collective per step, the flexible beta
in the outer CG folded into the r . z sum.  Iterations within a tenth of the undivided K-cycle's, the same solution, and
exactly the collectives the level plan predicts."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from util import rel_inf, sphere_points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _close(it, ref, slack=2):
    return abs(it - ref) <= max(slack, ref // 10)


def _build(f, w, pos, nrm, levels, kcycle=0, mixed=True, coarse_tol=1e-2):
    f.add_field_constraints(w)
    f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
    f.set_levels(levels, coarse_tol)
    f.set_multigrid(True)
    if mixed:
        f.set_mixed_precision(True)
    if kcycle:
        f.set_kcycle(kcycle)
    f.assemble()
    return f


@pytest.mark.parametrize("sizes,levels,kc,nranks", [([72, 64, 80], 3, 2, 3), ([320, 272], 4, 2, 4), ([96, 80, 64], 2, 1, 2)])
def test_loopback_group_runs_the_undivided_kcycle(fi, monkeypatch, sizes, levels, kc, nranks):
    """test_kcycle_preconditioner's shapes split into slabs: the group with the option set converges like the undivided
    K-cycle -- within a tenth of its iterations, to its solution -- and in fewer iterations than the group's V-cycle;
    FI_NO_KCYCLE takes it back to exactly the V-cycle's count."""
    rng = np.random.default_rng(3 * sum(sizes))
    pos, nrm = sphere_points(rng, sizes, 1500, noise=0.3)
    w = fi.Weights()
    tol = 1e-9
    one = _build(fi.LatticeField(sizes, dtype="f64"), w, pos, nrm, levels, kc)
    _, it_one, _ = one.solve_cg(None, 0, tol)
    gv = _build(fi.LatticeGroup(sizes, nranks, dtype="f64"), w, pos, nrm, levels)
    _, it_gv, _ = gv.solve_cg(None, 0, tol)
    gk = _build(fi.LatticeGroup(sizes, nranks, dtype="f64"), w, pos, nrm, levels, kc)
    _, it_gk, _ = gk.solve_cg(None, 0, tol)
    assert gk.stats()["converged"] == 1 and gk.true_residual() <= 1.5 * tol
    assert _close(it_gk, it_one), (it_gk, it_one)
    assert it_gk < it_gv, (it_gk, it_gv)
    assert rel_inf(gk.solution_f64(), one.solution_f64()) <= 2e-6
    monkeypatch.setenv("FI_NO_KCYCLE", "1")
    _, it_off, _ = gk.solve_cg(None, 0, tol)
    monkeypatch.delenv("FI_NO_KCYCLE")
    assert it_off == it_gv, (it_off, it_gv)


@pytest.mark.parametrize("sizes,nranks,levels,kc,pays,dtype,mixed", [([64, 64, 64], 8, 3, 3, True, "f32", False),
                                                                     ([64, 64, 64], 8, 3, 3, True, "f64", True),
                                                                     ([96, 96, 32], 8, 2, 1, False, "f64", True)])
def test_kcycle_with_a_replicated_tail(fi, sizes, nranks, levels, kc, pays, dtype, mixed):
    """64^3 in eight slabs (test_replicated_tail_of_a_slab_hierarchy): 32^3 is a slab K-level above the replicated 16^3 and
    8^3, whose junction sum it makes twice per visit.  96 x 96 x 32 in eight slabs: every coarse level is replicated, and the
    K-level 48 x 48 x 16 is corrected by each copy on its own.  The undivided lattice's levels, iterations and solution.
    (On the second, a hierarchy of two coarse levels, the K-cycle takes about twice the V-cycle's iterations on the undivided
    lattice as well -- the shallow-hierarchy case of fi_multigrid.hip's smoother notes: no comparison with the V-cycle there.)"""
    rng = np.random.default_rng(12)
    pos, nrm = sphere_points(rng, sizes, 4000)
    w = fi.Weights()
    tol = 1e-5 if dtype == "f32" else 1e-9
    one = _build(fi.LatticeField(sizes, dtype=dtype), w, pos, nrm, levels, kc, mixed=mixed, coarse_tol=1e-4)
    gv = _build(fi.LatticeGroup(sizes, nranks, dtype=dtype), w, pos, nrm, levels, mixed=mixed, coarse_tol=1e-4)
    gk = _build(fi.LatticeGroup(sizes, nranks, dtype=dtype), w, pos, nrm, levels, kc, mixed=mixed, coarse_tol=1e-4)
    assert gk.stats()["num_levels"] == one.stats()["num_levels"] == levels + 1
    _, it_one, r1 = one.solve_cg(None, 0, tol)
    _, it_gv, _ = gv.solve_cg(None, 0, tol)
    _, it_gk, rg = gk.solve_cg(None, 0, tol)
    assert r1 <= tol and rg <= tol and gk.true_residual() <= 1.5 * tol
    assert _close(it_gk, it_one), (it_gk, it_one)
    assert it_gk < it_gv or not pays, (it_gk, it_gv)
    assert rel_inf(gk.solution_f64(), one.solution_f64()) <= (2e-2 if dtype == "f32" else 2e-6)


@pytest.mark.parametrize("sizes,levels,kc,nranks", [([72, 64, 80], 3, 2, 3), ([64, 64, 64], 3, 3, 8), ([96, 96, 32], 2, 1, 8)])
def test_fp32_kcycle_without_a_replica(fi, monkeypatch, sizes, levels, kc, nranks):
    """fp32 CG and fp32 levels (no replica): the cycle runs on the CG's own contexts and uses their q as scratch, so the flexible
    beta must read A p_k from a vector the cycle does not touch.  The group takes the undivided K-cycle's iterations (+-2) and
    reaches its solution; FI_NO_KCYCLE gives exactly the group V-cycle's count.  (96 x 96 x 32 over 8 slabs: the K-level is
    replicated, every copy corrects on its own.)"""
    rng = np.random.default_rng(5 * sum(sizes) + nranks)
    pos, nrm = sphere_points(rng, sizes, 3000)
    w = fi.Weights()
    tol = 1e-5
    one = _build(fi.LatticeField(sizes, dtype="f32"), w, pos, nrm, levels, kc, mixed=False, coarse_tol=1e-4)
    gv = _build(fi.LatticeGroup(sizes, nranks, dtype="f32"), w, pos, nrm, levels, mixed=False, coarse_tol=1e-4)
    gk = _build(fi.LatticeGroup(sizes, nranks, dtype="f32"), w, pos, nrm, levels, kc, mixed=False, coarse_tol=1e-4)
    _, it_one, r1 = one.solve_cg(None, 0, tol)
    _, it_gv, _ = gv.solve_cg(None, 0, tol)
    _, it_gk, rg = gk.solve_cg(None, 0, tol)
    assert r1 <= tol and rg <= tol and gk.true_residual() <= 2 * tol     # (fp32: b - A x recomputed in fp32 drifts off the recurrence)
    assert abs(it_gk - it_one) <= 2, (it_gk, it_one, it_gv)
    assert rel_inf(gk.solution_f64(), one.solution_f64()) <= 1e-3
    monkeypatch.setenv("FI_NO_KCYCLE", "1")
    _, it_off, _ = gk.solve_cg(None, 0, tol)
    monkeypatch.delenv("FI_NO_KCYCLE")
    assert it_off == it_gv, (it_off, it_gv)


@pytest.mark.parametrize("group", [False, True])
def test_fp64_without_a_replica_has_no_kcycle_level(fi, group):
    """3-D fp64 levels have no fused recurrence step, so no level is a K-level: with the option set the solve is the plain
    V-cycle PCG -- the same iterations and the same bits -- on an undivided lattice and over slabs.  (From a caller's guess: the
    coarse-to-fine start's level solves keep the flexible beta whenever the option is set, fi_multigrid.hip cg_run_mg.)"""
    sizes = [64, 48, 56]
    rng = np.random.default_rng(31)
    pos, nrm = sphere_points(rng, sizes, 2500)
    w = fi.Weights()
    make = (lambda: fi.LatticeGroup(sizes, 4, dtype="f64")) if group else (lambda: fi.LatticeField(sizes, dtype="f64"))
    v = _build(make(), w, pos, nrm, 2, mixed=False, coarse_tol=1e-4)
    k = _build(make(), w, pos, nrm, 2, 2, mixed=False, coarse_tol=1e-4)
    guess = np.zeros(int(np.prod(sizes)), np.float32)
    _, itv, _ = v.solve_cg(guess, 0, 1e-9)
    _, itk, _ = k.solve_cg(guess, 0, 1e-9)
    assert itk == itv and np.array_equal(k.solution_f64(), v.solution_f64()), (itk, itv)


def _against_sample(x, g):
    sizes = [int(s) for s in g["sizes"]]
    stride = int(g["stride"])
    grid = np.asarray(x, np.float64).reshape(sizes[::-1])
    got = grid[tuple(slice(0, None, stride) for _ in sizes)]
    return float(np.abs(got - g["sample"]).max() / float(g["field_maxabs"]))


@pytest.mark.parametrize("config", [5, 3])
def test_field_rule_over_slabs_against_the_oracle(fi, capsys, config):
    """bench_settings' K-cycle solver for configs 5 (128^3) and 3 (1024^2) -- two levels less than at full size, the same
    coarsest lattice -- on a group of four slabs, stopped by the field rule: within 1e-5 of the oracle's fp64 solution, in
    the undivided solve's iterations."""
    from field_interpolation_amd import bench_settings as bs
    from field_interpolation_amd import synth
    s = bs.SETTINGS[config]
    if config == 5:
        g = np.load(os.path.join(GOLDEN, "config5_128_oracle_f64.npz"))
        sizes, w, pos, nrm = synth.config5(side=128, num_points=int(g["num_points"]), seed=int(g["seed"]))
    else:
        g = np.load(os.path.join(GOLDEN, "config3_1024_oracle_f64.npz"))
        sizes, w, pos, nrm = synth.config3(side=1024, points_per_shape=int(g["num_points"]) // 2, seed=2)
    assert sizes == [int(v) for v in g["sizes"]]
    runs = {}
    for name, f in (("one", fi.LatticeField(sizes, dtype="f64")), ("group", fi.LatticeGroup(sizes, 4, dtype="f64"))):
        f.add_field_constraints(w)
        bs.configure(f, s["levels"] - 2, s["coarse_tol"], by_field=True, kcycle=s["kcycle"], cheb=s.get("cheb"))
        f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
        f.assemble()
        _, it, _ = f.solve_cg(None, 0, s["tol"])
        runs[name] = (it, f.stats(), _against_sample(f.solution_f64(), g))
        del f
    (it1, _, err1), (itg, st, err) = runs["one"], runs["group"]
    with capsys.disabled():
        print("\n[config %d, K-cycle over 4 slabs, field rule] %d iterations (undivided %d), estimate %.2e, field error %.2e (undivided %.2e)"
              % (config, itg, it1, st["field_estimate"], err, err1))
    assert st["converged"] == 1 and st["field_rounds"] == 1 and 0 < st["field_estimate"] <= 1e-5
    assert err <= 1e-5
    assert _close(itg, it1), (itg, it1)


# ---- one slab per process ----------------------------------------------------------------------------------------------

def _level_plan(sizes, nranks, levels):
    """fi_levels.hip plan_levels: (unknowns, replicated) of coarse levels 1 .. L (slabs thinner than 4 planes: replicated)."""
    D = len(sizes)
    n = list(sizes)
    lo = [r * n[D - 1] // nranks for r in range(nranks)]
    hi = [(r + 1) * n[D - 1] // nranks for r in range(nranks)]
    plan, tail = [], False
    for _ in range(levels):
        n = [(v + 1) // 2 for v in n]
        if min(n) < 8:
            break
        if not tail:
            lo = [(v + 1) // 2 for v in lo]
            hi = [(v + 1) // 2 for v in hi]
            tail = any(h - l < 4 for l, h in zip(lo, hi))
        plan.append((int(np.prod(n)), tail))
    return plan


def _kcycle_collectives(sizes, nranks, levels, kcycle):
    """Collectives a K-cycle adds to one application of the preconditioner, from the level plan: one per flexible-CG step of a
    visit of a SLAB K-level (2 per visit), none on replicated ones, and the junction sum above the replicated tail once more per
    additional visit of its level.  K-levels: the first `kcycle` coarse levels that have a coarser one and that the undivided
    lattice does not run in the small-level engine (the coarsest levels of <= 4096 unknowns, at most 6 of them).  Only that
    rule: the fused-step and lumped-replica conditions of fi_multigrid.hip's kcycle_level are taken to hold (oriented points on
    3-D fp32 levels or 2-D levels, as in every case here) -- not an independent model of the K-level choice in general."""
    plan = _level_plan(sizes, nranks, levels)
    L = len(plan)
    engine, ok = [False] * L, True
    for k in reversed(range(L)):
        ok = ok and plan[k][0] <= 4096 and L - k <= 6
        engine[k] = ok
    visits, extra = 1, 0                                     # visits: corrections of level k + 1 per application
    for k in range(L):
        is_k = k + 1 <= kcycle and k + 1 < L and not engine[k]
        cycles = 2 * visits if is_k else visits              # its V-cycles
        if k + 1 < L and plan[k + 1][1] and not plan[k][1]:
            extra += cycles - 1                              # the junction: one vector sum per V-cycle of this level
        if is_k and not plan[k][1]:
            extra += 2 * visits
        visits = cycles
    return extra


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker_results(cases, nproc):
    env = dict(os.environ, FI_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", FI_WORKER_CASES=cases,
               FI_HIP_LIB=os.path.join(ROOT, "field_interpolation_amd", "libfi_hip_test.so"))
    r = None
    for _ in range(3):
        # (a port lost to somebody else between the probe and the rendezvous: EADDRINUSE, before any rank has touched the GPU)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "kcycle_rank_worker.py")]
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode == 0 or "EADDRINUSE" not in r.stderr:
            break
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULTS ")]
    assert line, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(line[-1][len("RESULTS "):])


def _check_processes(res, capsys):
    it = res["iterations"]
    assert len(set(it)) == 1, res                              # every rank stops in the same iteration
    assert res["num_levels"] == res["num_levels_one"], res
    assert _close(it[0], res["iterations_one"], 2 if res["nranks"] > 2 else 3), res
    assert min(res["converged"]) == 1, res
    assert max(res["true_rel"]) <= 1.5 * (res["tol"] if not res["by_field"] else max(res["rel"])) + 1e-12, res
    assert res["max_diff"] <= (5e-2 if res["tol"] >= 1e-6 else 1e-4), res
    # the collectives: K-cycle and V-cycle run the same count of iterations; the difference is the level plan's prediction
    # per application of the preconditioner (one per iteration but the last, one at the start)
    n = res["count_iterations"]
    assert res["iterations_k"] == [n] * res["nranks"] and res["iterations_v"] == [n] * res["nranks"], res
    extra = _kcycle_collectives(res["sizes"], res["nranks"], res["levels"], res["kcycle"])
    assert extra > 0
    for rk, rv in zip(res["reductions_k"], res["reductions_v"]):
        assert rk - rv == extra * n, (rk, rv, extra, res)
    with capsys.disabled():
        print("\n[%s] %d iterations (undivided %d), %.2f collectives per iteration; %d more per cycle than the V-cycle's"
              % (res["case"], it[0], res["iterations_one"], res["reductions"][0] / max(it[0], 1), extra))


def test_two_processes_kcycle(capsys):
    results = _worker_results("pair", 2)
    assert len(results) == 2
    for res in results:
        _check_processes(res, capsys)


def test_four_processes_kcycle_with_a_replicated_tail(capsys):
    results = _worker_results("tail", 4) + _worker_results("config5", 4)
    assert len(results) == 3
    for res in results:
        _check_processes(res, capsys)
        assert min(res["points_kept"]) == res["points"], res    # the replicated levels are assembled from every point
    c5 = results[-1]
    assert c5["by_field"] and c5["field_rounds"] == [1] * 4 and 0 < max(c5["field_estimate"]) <= 1e-5, c5


def test_kcycle_on_a_rank_without_points(capsys):
    """Rank 1 holds no points: it must pick the same K-levels and run the same collectives as rank 0."""
    results = _worker_results("lopsided", 2)
    assert len(results) == 1
    res = results[0]
    assert res["points_kept"][1] == 0 and res["points_kept"][0] == res["points"], res
    _check_processes(res, capsys)


def test_config5_full_size_on_eight_slabs(fi, capsys):
    """Config 5 at 512^3 with bench_settings' solver (7 levels, K-cycle on 4, smoother (4, 10)) as a loop-back group of eight
    slabs: converged, in the undivided K-cycle's iterations (+-3) at the same residual."""
    from field_interpolation_amd import bench_settings as bs
    from field_interpolation_amd import synth
    s = bs.SETTINGS[5]
    sizes, w, pos, nrm = synth.config5()
    its = {}
    for name, f in (("one", bs.headline_field(fi, 5, sizes, w)), ("group", fi.LatticeGroup(sizes, 8, dtype="f64"))):
        if name == "group":
            f.add_field_constraints(w)
            bs.configure(f, s["levels"], s["coarse_tol"], kcycle=s["kcycle"], cheb=s["cheb"])
        f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
        f.assemble()
        _, it, rel = f.solve_cg(None, 0, s["tol"])
        st = f.stats()
        its[name] = it
        assert st["converged"] == 1 and st["num_levels"] == 7, st
        with capsys.disabled():
            print("\n[config 5 at 512^3, K-cycle, %s] %d iterations, residual %.2e, solve %.1f ms" % (name, it, rel, st["solve_ms"]))
        del f
    assert abs(its["group"] - its["one"]) <= 3, its
