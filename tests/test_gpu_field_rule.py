"""The field stop rule (FI_OPT_FIELD_TOLERANCE, include/fi_hip.h) against the ORACLE's fp64 solution -- not the GPU's own
solve -- on every solver path it runs on, and what fi_stats reports about a solve on every path, the rule's or not.

  (a) designed cases over lattice shapes (1-D, 2-D, 3-D, odd sides, a 48^3 SDF), data kinds (value rows with either value
      kernel, oriented points with each gradient kernel), weights, solvers (fp64 V-cycle, fp64 CG + fp32 V-cycle, K-cycle
      on 1 and 2 levels, an fp32 context), tolerances, starts (cold, a smooth bump, the oracle's own solution) and slab
      counts (2, 3 and 16 = kFieldRanks): stopped by the field, with an estimate within the tolerance and a true error
      within twice it (the margin fi_hip.h describes);
  (b) field_rounds is 1 only when the field test ended the solve (not max_iterations, not the precision's floor);
  (c) the field stats after a Jacobi-PCG, a polynomial-PCG and a residual-rule V-cycle solve are not the previous solve's;
  (d) paths the rule cannot run on stop by the residual at the caller's tolerance and say so.
"""
import os

import numpy as np
import pytest

from util import build_pair, oracle_weights, rel_inf, sphere_points

pytestmark = pytest.mark.gpu

EXACT_FLOPS = 2e10      # banded Cholesky costs about n bw^2, bw about twice the product of the fast axes
ORACLE_PCG_TOL = 1e-12


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _threads():
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", "16"))
    except ValueError:
        n = 16
    return max(1, min(16, n))


def _oracle_solve(fo, sizes):
    n = int(np.prod(sizes))
    bw = 2 * int(np.prod(sizes[:-1])) if len(sizes) > 1 else 4
    if n * float(bw) ** 2 <= EXACT_FLOPS:
        x = fo.solve_exact_f64()
        assert x is not None
        return np.asarray(x, np.float64), "exact"
    res = fo.solve_pcg_f64_mt(None, 0, ORACLE_PCG_TOL, threads=_threads())
    assert res is not None
    x, it, _ = res
    atb = fo.apply_transpose_rhs()
    true_rel = np.linalg.norm(atb - fo.apply_normal(x)) / np.linalg.norm(atb)
    assert true_rel <= 2 * ORACLE_PCG_TOL, true_rel     # the oracle's own iterate, checked through A^T (A x)
    return np.asarray(x, np.float64), "pcg %d it" % it


# (id, sizes, data, weights, solver, tol, start, slabs)
#   data: "value" (value_kernel 1), "value_nn" (value_kernel 0: value rows need the normals), "sdf<k>" (oriented points,
#   gradient_kernel k); solver: "f64" (fp64 V-cycle: Chebyshev in the full operator), "mixed" (fp64 CG + fp32 V-cycle:
#   the polynomial smoother on 3-D levels), "k1" / "k2" (K-cycle on 1 / 2 levels), "f32" (an fp32 context);
#   start: "cold" (coarse-to-fine), "bump" (the oracle's solution off by a smooth bump of 50 x tol), "oracle" (the oracle's
#   solution rounded to fp32); slabs: 0 = undivided, else a LatticeGroup of that many slabs
CASES = [
    ("2d-value-f64",          [200, 136],    "value",    dict(model_2=0.5),                "f64",   1e-5, "cold",   0),
    ("2d-odd-sdf1-mixed",     [97, 161],     "sdf1",     dict(model_1=0.2, model_2=0.6),   "mixed", 1e-6, "cold",   0),
    ("2d-sdf0-k1",            [200, 136],    "sdf0",     dict(model_2=0.5),                "k1",    1e-5, "cold",   0),
    ("2d-odd-value_nn-f32",   [97, 161],     "value_nn", dict(model_0=0.005, model_2=0.5), "f32",   1e-4, "cold",   0),
    ("2d-odd-sdf2-oracle",    [97, 161],     "sdf2",     dict(model_2=0.5),                "f64",   1e-4, "oracle", 0),
    ("3d-value-f64",          [24, 20, 28],  "value",    dict(model_1=0.1, model_2=0.5),   "f64",   1e-6, "cold",   0),
    ("3d-sdf2-mixed",         [24, 20, 28],  "sdf2",     dict(model_2=0.5),                "mixed", 1e-5, "cold",   0),
    ("3d-value_nn-f64-bump",  [24, 20, 28],  "value_nn", dict(model_0=0.005, model_2=0.5), "f64",   1e-4, "bump",   0),
    ("3d-odd-sdf1-mixed-bump", [33, 30, 35], "sdf1",     dict(model_2=0.5),                "mixed", 1e-5, "bump",   0),
    ("3d-odd-value-k2",       [33, 30, 35],  "value",    dict(model_1=0.1, model_2=0.5),   "k2",    1e-4, "cold",   0),
    ("3d-odd-value-f32",      [33, 30, 35],  "value",    dict(model_2=0.5),                "f32",   1e-3, "cold",   0),
    ("48cube-sdf1-mixed",     [48, 48, 48],  "sdf1",     dict(model_2=0.5),                "mixed", 1e-5, "cold",   0),
    ("48cube-sdf1-k1-oracle", [48, 48, 48],  "sdf1",     dict(model_2=0.5),                "k1",    1e-5, "oracle", 0),
    ("1d-value-f64",          [300],         "value",    dict(model_1=0.1, model_2=0.5),   "f64",   1e-6, "cold",   0),
    ("2d-value-mixed-2slabs", [200, 136],    "value",    dict(model_1=0.1, model_2=0.5),   "mixed", 1e-5, "cold",   2),
    ("3d-odd-sdf0-f64-3slabs-bump", [33, 30, 35], "sdf0", dict(model_0=0.005, model_2=0.5), "f64", 1e-5, "bump",   3),
    ("2d-value-mixed-16slabs", [128, 512],   "value",    dict(model_2=0.5),                "mixed", 1e-5, "cold",  16),
]
CASE_BY_ID = {c[0]: c for c in CASES}


def _inputs(fi, case):
    cid, sizes, data, kw, solver, tol, start, slabs = case
    rng = np.random.default_rng(sum(ord(ch) for ch in cid))
    n = int(np.prod(sizes))
    npts = int(min(3000, max(300, n // 20)))
    if len(sizes) == 1:
        pos = rng.uniform(0.0, sizes[0] - 1.0, (npts, 1)).astype(np.float32)
        nrm = np.where(rng.random((npts, 1)) < 0.5, -1.0, 1.0).astype(np.float32)
    else:
        pos, nrm = sphere_points(rng, sizes, npts, noise=0.4)
    if data.startswith("sdf"):
        w = fi.Weights(gradient_kernel=fi.GradientKernel(int(data[3:])), **kw)
        return w, pos, nrm, None
    val = rng.normal(size=npts).astype(np.float32)
    if data == "value_nn":
        return fi.Weights(data_gradient=0.0, value_kernel=fi.ValueKernel(0), **kw), pos, nrm, val
    return fi.Weights(data_gradient=0.0, **kw), pos, None, val


def _configure(f, solver, tol, levels=3):
    f.set_levels(levels, 1e-3)
    f.set_multigrid(True)
    if solver in ("mixed", "k1", "k2"):
        f.set_mixed_precision(True)
    if solver in ("k1", "k2"):
        f.set_kcycle(int(solver[1]))
    f.set_field_tolerance(tol)


def _bump(sizes, x_ref, amplitude):
    grid = np.meshgrid(*[np.linspace(0.0, np.pi, n_) for n_ in sizes[::-1]], indexing="ij")
    bump = np.ones_like(grid[0])
    for gcoord in grid:
        bump = bump * np.sin(gcoord)
    return (x_ref + amplitude * float(np.abs(x_ref).max()) * bump.reshape(-1)).astype(np.float32)


@pytest.fixture(scope="module")
def references(oracle, fi):
    """The oracle's fp64 solution of each designed case, computed once (keyed by case id)."""
    cache = {}

    def get(case):
        if case[0] not in cache:
            w, pos, nrm, val = _inputs(fi, case)
            fo, _ = build_pair(oracle, fi, case[1], w, pos, nrm, None, val, dtype="f64")
            cache[case[0]] = _oracle_solve(fo, case[1])
        return cache[case[0]]
    return get


def _build_gpu(fi, case, group_slabs=0):
    cid, sizes, data, kw, solver, tol, start, slabs = case
    w, pos, nrm, val = _inputs(fi, case)
    dtype = "f32" if solver == "f32" else "f64"
    f = fi.LatticeGroup(sizes, group_slabs, dtype=dtype) if group_slabs else fi.LatticeField(sizes, dtype=dtype)
    f.add_field_constraints(w)
    f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None, values=val)
    _configure(f, solver, tol)
    f.assemble()
    return f


@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_field_rule_against_the_oracle(fi, references, cid, capsys):
    case = CASE_BY_ID[cid]
    _, sizes, data, kw, solver, tol, start, slabs = case
    x_ref, how = references(case)
    guess = None
    if start == "bump":
        guess = _bump(sizes, x_ref, 50.0 * tol)
    elif start == "oracle":
        guess = x_ref.astype(np.float32)
    runs = [("undivided", _build_gpu(fi, case))]
    if slabs:
        runs.append(("%d slabs" % slabs, _build_gpu(fi, case, slabs)))
    got = []
    for name, f in runs:
        res = f.solve_cg(guess, 4000, 1e-5)     # (the rule ignores the residual tolerance)
        assert res is not None, (cid, name, "breakdown")
        st = f.stats()
        err = rel_inf(f.solution_f64(), x_ref)
        with capsys.disabled():
            print("\n[field rule %s, %s; oracle %s] %d iterations, estimate %.2e, true error %.2e, error / tol %.3f, "
                  "error / estimate %.3f" % (cid, name, how, st["iterations"], st["field_estimate"], err, err / tol,
                                             err / st["field_estimate"] if st["field_estimate"] > 0 else float("nan")))
        assert st["converged"] == 1, (cid, name, st)
        assert st["field_rounds"] == 1, (cid, name, st)
        assert 0 < st["field_estimate"] <= tol, (cid, name, st)
        assert err <= 2 * tol, (cid, name, err, st)
        got.append(st["iterations"])
    if slabs:
        it1, itg = got
        assert abs(itg - it1) <= max(2, it1 // 10), (cid, got)


def _value_inputs(fi, sizes, seed, npts, kw=None):
    rng = np.random.default_rng(seed)
    pos, _ = sphere_points(rng, sizes, npts, noise=0.4)
    val = rng.normal(size=npts).astype(np.float32)
    return fi.Weights(data_gradient=0.0, **(kw or dict(model_2=0.5))), pos, val


def _value_problem(oracle, fi, sizes, dtype, seed, npts=400, kw=None):
    w, pos, val = _value_inputs(fi, sizes, seed, npts, kw)
    return build_pair(oracle, fi, sizes, w, pos, None, None, val, dtype=dtype)


def test_field_rounds_means_stopped_by_the_field(oracle, fi, capsys):
    sizes = [40, 36]
    rng = np.random.default_rng(5)
    pos, nrm = sphere_points(rng, sizes, 500)
    w = fi.Weights()
    fo, f = build_pair(oracle, fi, sizes, w, pos, nrm, None, None, dtype="f64")
    x_ref = fo.solve_exact_f64()
    _configure(f, "f64", 1e-6, levels=2)
    f.assemble()
    # the iteration cap ends a solve under the rule: not stopped by the field
    f.solve_cg(None, 2, 0.0)
    st = f.stats()
    assert st["iterations"] == 2 and st["converged"] == 0 and st["field_rounds"] == 0, st
    # a tolerance below what fp64 can certify: the recurrence's floor (1e-13) ends the solve -- converged (as converged as
    # the arithmetic allows), but not by the field
    f.set_field_tolerance(1e-15)
    f.solve_cg(None, 4000, 0.0)
    st = f.stats()
    err64 = rel_inf(f.solution_f64(), x_ref)
    assert st["converged"] == 1 and st["field_rounds"] == 0 and st["stop_residual"] <= 1e-13, st
    assert err64 <= 1e-6, err64
    # an fp32 context asked for 1e-8: its floor (2e-7) or the cap ends the solve; the estimate says it is not certified
    fo32, g = _value_problem(oracle, fi, sizes, "f32", 6)
    x32_ref = fo32.solve_exact_f64()
    _configure(g, "f32", 1e-8, levels=2)
    g.assemble()
    g.solve_cg(None, 400, 0.0)
    st = g.stats()
    err32 = rel_inf(g.solution_f64(), x32_ref)
    with capsys.disabled():
        print("\n[field_rounds] fp64 at the floor: %d iterations, residual %.1e, error %.1e; fp32 asked for 1e-8: %d iterations, "
              "estimate %.2e, residual %.1e, error against the oracle %.2e" % (
                  f.stats()["iterations"], f.stats()["stop_residual"], err64, st["iterations"], st["field_estimate"],
                  st["stop_residual"], err32))
    assert st["converged"] == 0 and st["field_rounds"] == 0, st
    assert not (0.0 <= st["field_estimate"] <= 1e-8), st
    assert err32 <= 1e-4, err32      # what fp32 allows: the field still converged as far as its arithmetic goes


def _residual_rule_reported(st):
    assert st["field_estimate"] == -1.0, st
    assert st["field_per_residual"] == 0.0, st
    assert st["field_rounds"] == 0, st
    assert st["stop_residual"] == st["rel_residual"], st


def test_stats_after_every_solver_path(oracle, fi):
    sizes = [24, 20, 28]
    fo, f = _value_problem(oracle, fi, sizes, "f64", 7, npts=600, kw=dict(model_1=0.1, model_2=0.5))
    x_ref = fo.solve_exact_f64()
    assert f.stats()["field_estimate"] == -1.0            # a fresh context: no solve, none by the field
    _configure(f, "f64", 1e-5)
    f.assemble()
    assert f.stats()["field_estimate"] == -1.0 and f.stats()["num_levels"] >= 2
    # 1. by the field
    f.solve_cg(None, 0, 1e-5)
    st = f.stats()
    assert st["field_rounds"] == 1 and 0 < st["field_estimate"] <= 1e-5 and st["field_per_residual"] > 0, st
    assert rel_inf(f.solution_f64(), x_ref) <= 2e-5
    # 2. Jacobi-PCG (multigrid off; the field tolerance is still set: this path falls back to the residual rule)
    f.set_multigrid(False)
    f.solve_cg(None, 0, 1e-7)
    st = f.stats()
    _residual_rule_reported(st)
    assert st["converged"] == 1 and st["rel_residual"] <= 1e-7 and st["prec_samples"] == 0, st
    # 3. polynomial PCG (multigrid still off)
    f.set_polynomial(4)
    f.solve_cg(None, 0, 1e-7)
    st = f.stats()
    _residual_rule_reported(st)
    assert st["converged"] == 1 and st["rel_residual"] <= 1e-7 and st["prec_samples"] > 0, st
    # 4. V-cycle PCG under the residual rule
    f.set_polynomial(0)
    f.set_multigrid(True)
    f.set_field_tolerance(0)
    f.solve_cg(None, 0, 1e-7)
    st = f.stats()
    _residual_rule_reported(st)
    assert st["converged"] == 1 and st["rel_residual"] <= 1e-7, st
    assert rel_inf(f.solution_f64(), x_ref) <= 1e-4


def _check_residual_rule(fo, f, tol, label):
    """A solve with a field tolerance set, on a path without the rule: stopped by the residual at the caller's `tol` (in
    the GPU's own b - A x and in the oracle's equations), and the stats say so."""
    st = f.stats()
    _residual_rule_reported(st)
    assert st["converged"] == 1, (label, st)
    assert st["stop_residual"] <= tol, (label, st)
    assert st["stop_residual"] > 1e-10, (label, st)     # the caller's tolerance, not the rule's fp64 floor (1e-13)
    assert f.true_residual() <= 1.01 * tol, label
    x = f.solution_f64()
    atb = fo.apply_transpose_rhs()
    oracle_rel = np.linalg.norm(atb - fo.apply_normal(x)) / np.linalg.norm(atb)
    assert oracle_rel <= 1.05 * tol, (label, oracle_rel)


def test_field_tolerance_on_paths_without_the_rule(oracle, fi):
    tol = 1e-4
    # a lattice too small for a coarser level
    fo, f = _value_problem(oracle, fi, [20, 9], "f64", 8, npts=60)
    _configure(f, "f64", 1e-9, levels=4)
    f.assemble()
    assert f.stats()["num_levels"] == 1
    f.solve_cg(None, 0, tol)
    _check_residual_rule(fo, f, tol, "[20, 9]")
    # hand-built rows: no geometry to coarsen
    fo, f = _value_problem(oracle, fi, [64, 64], "f64", 9)
    fo.add_equation(1.0, 2.0, [(7, 1.0)])
    f.add_rows_coo(np.array([0]), np.array([7]), np.array([1.0], np.float32), np.array([2.0], np.float32))
    _configure(f, "f64", 1e-9, levels=2)
    f.assemble()
    assert f.stats()["num_levels"] == 1
    f.solve_cg(None, 0, tol)
    _check_residual_rule(fo, f, tol, "add_rows_coo")
    # multigrid off (levels built: a coarse-to-fine start, then Jacobi-PCG)
    fo, f = _value_problem(oracle, fi, [97, 161], "f64", 10)
    _configure(f, "f64", 1e-9, levels=2)
    f.set_multigrid(False)
    f.assemble()
    f.solve_cg(None, 0, tol)
    _check_residual_rule(fo, f, tol, "multigrid off")
    # more slabs than the rule's kFieldRanks = 16
    sizes = [128, 544]
    w, pos, val = _value_inputs(fi, sizes, 11, 2000)
    fo = oracle.LatticeField(sizes)
    fo.add_field_constraints(oracle_weights(oracle, w))
    for p, v in zip(pos, val):
        fo.add_value_constraint(p, float(v), float(np.float32(w.data_pos)))
    g = fi.LatticeGroup(sizes, 17, dtype="f64")
    g.add_field_constraints(w)
    g.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, None, None, values=val)
    _configure(g, "f64", 1e-9, levels=2)
    g.assemble()
    g.solve_cg(None, 0, tol)
    _check_residual_rule(fo, g, tol, "17 slabs")
