"""Robust fits on the device (fi_robust.hip through fi_point_residuals / fi_robust_reweight / fi_solve_robust) against the
numpy restatement of the contract (tests/robust_reference.py): residuals, scale, weight factors and point weights bit for
bit; the reweighted context is the reweighted problem; the loop agrees with the fp64 reference loop on the oracle's exact
solver and recovers the truth from data with gross errors."""
import numpy as np
import pytest

import robust_reference as R

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(got, want, what=""):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


def _context(fi, sizes, dtype, batches, weights=None):
    f = fi.LatticeField(sizes, dtype=dtype)
    f.add_field_constraints(weights if weights is not None else fi.Weights(model_2=1.0))
    for b in batches:
        if b["prior"]:
            f.add_border_prior(float(b["vw"]))
        else:
            f.add_points(float(b["vw"]), b["vk"], float(b["gw"]), b["gk"], b["pos"], b["nrm"], b["pw"], b["val"])
    return f


def _edge_points(sizes, n, rng):
    """random points over the lattice and a little beyond; exact lattice positions; negative coordinates above -1; the last
    lattice point; outside; NaN"""
    gn = np.asarray(sizes, np.float64)
    D = len(sizes)
    p = rng.uniform(-0.9, 1.0, size=(n, D)) * 0.0 + rng.random((n, D)) * (gn - 1.0)
    p[0] = gn - 1.0
    p[1] = 0.0
    p[2:22] = np.round(p[2:22])
    p[22:40] = np.floor(p[22:40]) + 0.5
    p[40:60, 0] = -rng.random(20) * 0.99
    p[60:70] = -rng.random((10, D)) * 0.99
    p[70:80, -1] = gn[-1] - 1.0 + rng.random(10) * 0.9
    p[80:84, 0] = gn[0] + 2.5
    p[84:86, -1] = -1.25
    p[86, 0] = np.nan
    p[87, -1] = np.inf
    return p.astype(F)


def _two_batches(sizes, variant, rng, n=300):
    D = len(sizes)
    pa, pb = _edge_points(sizes, n, rng), _edge_points(sizes, n, rng)
    nrm = lambda: rng.normal(size=(n, D)).astype(F)  # noqa: E731
    val = lambda: rng.normal(size=n).astype(F)       # noqa: E731
    pw = rng.uniform(0.2, 2.0, n).astype(F)
    pw[::7] = 0.0
    if variant == 0:
        a = R.batch(pa, nrm=nrm(), pw=pw, val=val(), vw=0.7, vk=R.VALUE_NEAREST, gw=0.3, gk=R.GRAD_NEAREST)
        b = R.batch(pb, val=val(), vw=1.3, vk=R.VALUE_LINEAR)
    else:
        a = R.batch(pa, nrm=nrm(), vw=0.6, vk=R.VALUE_LINEAR, gw=1.7, gk=R.GRAD_CELL_EDGES)
        b = R.batch(pb, nrm=nrm(), pw=pw, val=val(), vw=0.9, vk=R.VALUE_LINEAR, gw=0.0, gk=R.GRAD_NEAREST)
    return [a, b, R.batch(np.zeros((0, D)), vw=0.25, prior=True)]


LATTICES = [[33], [2, 2], [17, 13], [3, 2, 2], [9, 8, 7]]


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("sizes", LATTICES, ids=lambda s: "x".join(map(str, s)))
def test_residuals_bit_for_bit(fi, sizes, dtype, variant):
    rng = np.random.default_rng(sum(sizes) * 7 + variant)
    batches = _two_batches(sizes, variant, rng)
    f = _context(fi, sizes, dtype, batches)
    assert f.point_count() == 600                                    # the border prior's rows are not data points
    x = rng.normal(size=int(np.prod(sizes))).astype(F)               # not a solution
    want = R.residuals(sizes, batches, x, np.float64 if dtype == "f64" else np.float32)
    got = f.point_residuals(x)
    assert (want < 0).sum() >= 10 and (want >= 0).sum() >= 300
    _same(got, want, "residuals")
    # one step on top: scale, omega
    om, s = f.robust_reweight(x, loss="cauchy")
    assert _bits([s])[0] == _bits([R.scale(want)])[0]
    _same(om, R.omega(R.CAUCHY, want, R.scale(want)), "omega")
    # the residuals are measured from the caller's weights, whatever the step has put under the rows
    _same(f.point_residuals(x), want, "residuals after the step")


_BIG = {}


def _big(n_out):
    if n_out not in _BIG:
        sizes = [64, 64, 64]
        rng = np.random.default_rng(100 + n_out)
        n = 200000
        pos = (rng.random((n, 3)) * 63.0).astype(F)
        pos[:n_out, 1] = 70.0                                          # outside: M = n - n_out
        val = rng.normal(size=n).astype(F)
        pw = rng.uniform(0.5, 1.5, n).astype(F)
        b = R.batch(pos, val=val, pw=pw, vw=0.8, vk=R.VALUE_LINEAR)
        x = rng.normal(size=64 ** 3).astype(F)
        _BIG[n_out] = (sizes, b, x, R.residuals(sizes, [b], x, np.float32))
    return _BIG[n_out]


@pytest.mark.parametrize("loss,tuning,scale,n_out", [("huber", 0.0, 0.0, 3), ("cauchy", 0.0, 0.0, 4), ("tukey", 3.0, 0.0, 3),
                                                     ("tukey", 0.0, 0.0, 4), ("huber", 0.0, 0.07, 4)])
def test_beyond_one_workgroup_and_the_sorts_threshold(fi, loss, tuning, scale, n_out):
    sizes, b, x, want = _big(n_out)
    assert (want >= 0).sum() == 200000 - n_out
    f = _context(fi, sizes, "f32", [b])
    _same(f.point_residuals(x), want, "residuals")
    om, s = f.robust_reweight(x, loss=loss, tuning=tuning, scale=scale)
    s_want = F(scale) if scale > 0 else R.scale(want)
    assert _bits([s])[0] == _bits([s_want])[0], (s, s_want)
    om_want = R.omega(loss, want, s_want, tuning)
    _same(om, om_want, "omega")
    assert 0.05 < (om_want < 1).mean() and np.all(om_want[:n_out] == 1)
    # the point weights under the rows: the context is the one a caller builds from base * sqrt(omega)
    g = _context(fi, sizes, "f32", R.with_weights([b], R.point_weights(b["pw"], om_want)))
    assert np.array_equal(f.Atb(), g.Atb())


def _mixed_batches(sizes, rng, n=400):
    D = len(sizes)
    gn = np.asarray(sizes, np.float64)
    pa = (rng.random((n, D)) * (gn - 1.0)).astype(F)
    pb = (rng.random((n, D)) * (gn - 1.0)).astype(F)
    pw = rng.uniform(0.3, 1.8, n).astype(F)
    a = R.batch(pa, nrm=rng.normal(size=(n, D)), pw=pw, vw=0.7, vk=R.VALUE_NEAREST, gw=0.4, gk=R.GRAD_CELL_EDGES)
    b = R.batch(pb, val=rng.normal(size=n), vw=1.1, vk=R.VALUE_LINEAR)
    return [a, b]


@pytest.mark.parametrize("levels", [0, 1])
@pytest.mark.parametrize("sizes", [[17, 13], [9, 8, 7]], ids=lambda s: "x".join(map(str, s)))
def test_the_reweighted_context_is_the_reweighted_problem(fi, sizes, levels):
    rng = np.random.default_rng(sum(sizes) + levels)
    batches = _mixed_batches(sizes, rng)
    ntot = int(np.prod(sizes))
    x = rng.normal(size=ntot).astype(F)

    def make(bs):
        f = _context(fi, sizes, "f64", bs)
        if levels:
            f.set_levels(levels)
            f.set_multigrid(True)
        return f

    f = make(batches)
    atb0 = f.Atb()
    om, s = f.robust_reweight(x, loss="cauchy")
    assert s > 0 and (om < 0.9).sum() > 50
    want = R.residuals(sizes, batches, x, np.float64)
    _same(om, R.omega(R.CAUCHY, want, R.scale(want)), "omega")
    g = make(R.with_weights(batches, R.point_weights(R.base_weights(batches), om)))
    probe = rng.normal(size=ntot)
    assert np.array_equal(f.Atb(), g.Atb()) and not np.array_equal(f.Atb(), atb0)
    assert np.array_equal(f.diag(), g.diag())
    assert np.array_equal(f.apply_AtA(probe), g.apply_AtA(probe))
    if levels:
        guess = rng.normal(size=ntot).astype(F)
        xf, itf, _ = f.solve_cg(guess=guess, error_tolerance=1e-9)
        xg, itg, _ = g.solve_cg(guess=guess, error_tolerance=1e-9)
        assert itf == itg and itf > 1
        _same(xf, xg, "solutions")
    # every reweighting starts from the caller's weights, not from the last omega
    om2, s2 = f.robust_reweight(x, loss="cauchy")
    _same(om2, om, "second step")
    assert s2 == s
    f.reset_point_weights()
    assert np.array_equal(f.Atb(), atb0)


def test_scale_zero_changes_nothing(fi):
    sizes = [12, 11]
    rng = np.random.default_rng(3)
    x = rng.normal(size=132).astype(F)
    n = 200
    ij = np.stack([rng.integers(0, 12, n), rng.integers(0, 11, n)], axis=1)
    pos = ij.astype(F)
    val = x[ij[:, 0] + 12 * ij[:, 1]].copy()
    pos[120:] += rng.random((80, 2)).astype(F) * 0.9 * (pos[120:] < 10)     # 40 % off the lattice points, with other values
    val[120:] += 1.0
    b = R.batch(pos, val=val, vw=1.0, vk=R.VALUE_LINEAR)
    want = R.residuals(sizes, [b], x)
    assert (want == 0).sum() >= 120 and (want > 0).sum() > 50 and R.scale(want) == 0
    f = _context(fi, sizes, "f32", [b])
    atb0 = f.Atb()
    om, s = f.robust_reweight(x, loss="tukey")
    assert s == 0 and np.all(om == 1)
    assert np.array_equal(f.Atb(), atb0)
    # a field the solver reproduces exactly: constant data on lattice points under a model that ignores constants; the
    # start is the solution, its residual is exactly zero
    f = _context(fi, sizes, "f64", [R.batch(pos[:120], val=np.full(120, 0.5), vw=1.0, vk=R.VALUE_LINEAR)])
    field, om, st = f.solve_robust(guess=np.full(132, 0.5, F), loss="huber", rounds=5, error_tolerance=1e-10)
    assert np.all(field == F(0.5))
    assert st["rounds"] == 0 and st["scale"] == 0 and st["max_weight_change"] == 0 and np.all(om == 1)
    assert st["points_used"] == 120 and st["points_zeroed"] == 0


# ---- end to end ------------------------------------------------------------------------------------------
CASES = {"3d": ([24, 20, 16], 6000, 1.0), "2d": ([64, 64], 3000, 3.0)}
_REF = {}


def _reference(name):
    """the inputs of tests/test_robust_reference.py (seed 1) and the fp64 reference loop on them, computed once"""
    if name not in _REF:
        from oracle import fi_oracle
        sizes, npoints, model_2 = CASES[name]
        b, bad = R.noisy_value_data(sizes, npoints, 1)
        x, om, fields = R.irls(sizes, fi_oracle.Weights(model_2=model_2), [b], loss=R.HUBER, rounds=5)
        _REF[name] = dict(sizes=sizes, model_2=model_2, batch=b, bad=bad, x=x, omega=om, plain=fields[0],
                          truth=R.truth_on_lattice(sizes))
    return _REF[name]


def _dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name,solver", [("2d", "plain"), ("3d", "plain"), ("3d", "vcycle-mixed")])
def test_end_to_end_fp64(fi, name, solver):
    ref = _reference(name)
    sizes, b = ref["sizes"], ref["batch"]

    def make():
        f = _context(fi, sizes, "f64", [b], fi.Weights(model_2=ref["model_2"]))
        if solver != "plain":
            f.set_levels(1)
            f.set_multigrid(True)
            f.set_mixed_precision(True)
        return f

    f = make()
    plain, it0, _ = f.solve_cg(error_tolerance=1e-10)
    field, om, st = f.solve_robust(loss="huber", rounds=5, weight_tolerance=0.0, error_tolerance=1e-10)
    d = _dist(f.solution_f64(), ref["x"])
    e_plain, e_robust = R.rms(plain, ref["truth"]), R.rms(field, ref["truth"])
    print("%s %s: distance to the reference loop %.3g; rms error plain %.4f robust %.4f; %s" % (name, solver, d, e_plain, e_robust, st))
    assert d <= 1e-5, d
    assert e_robust <= 0.25 * e_plain, (e_plain, e_robust)
    assert st["rounds"] == 5 and st["points_used"] == len(b["pos"]) and st["scale"] > 0
    assert np.abs(om - ref["omega"]).max() < 1e-3      # (the fields agree to 1e-5 at most: not bit for bit)
    assert om[ref["bad"]].mean() < 0.2 < 0.8 < om[~ref["bad"]].mean()
    # the iterations are those of all solves: a loop of one round is the plain solve and the solve stats() reports
    g = make()
    _, _, st1 = g.solve_robust(loss="huber", rounds=1, error_tolerance=1e-10)
    assert st1["rounds"] == 1 and st1["iterations"] == it0 + g.stats()["iterations"]
    assert st["iterations"] > st1["iterations"]
    # afterwards the context holds the robust system: its own solution has no residual there
    assert f.true_residual() < 1e-8


def test_end_to_end_fp32(fi):
    """fp32 context, 3-D shape.  The robust field may be 4x as far from the fp64 reference loop as the plain fp32 solve is
    from the oracle's exact solve of the same system (round 0: what a solve gave before robust fits existed)."""
    ref = _reference("3d")
    sizes, b = ref["sizes"], ref["batch"]
    f = _context(fi, sizes, "f32", [b], fi.Weights(model_2=ref["model_2"]))
    plain, _, _ = f.solve_cg(error_tolerance=1e-6)
    d0 = _dist(plain, ref["plain"])
    field, om, st = f.solve_robust(loss="huber", rounds=5, error_tolerance=1e-6)
    d = _dist(field, ref["x"])
    print("fp32: plain solve to the exact solve %.3g, robust field to the reference loop %.3g (%s)" % (d0, d, st))
    assert st["rounds"] == 5
    assert d <= 4 * d0, "plain fp32 solve to the exact solve: %.3g; robust field to the reference loop: %.3g" % (d0, d)
    assert R.rms(field, ref["truth"]) <= 0.25 * R.rms(plain, ref["truth"])


def test_early_stop(fi):
    ref = _reference("2d")
    f = _context(fi, ref["sizes"], "f64", [ref["batch"]], fi.Weights(model_2=ref["model_2"]))
    _, _, st = f.solve_robust(loss="huber", rounds=20, weight_tolerance=1e-3, error_tolerance=1e-10)
    print(st)
    assert 1 <= st["rounds"] < 20 and st["max_weight_change"] < 1e-3


def test_refusals(fi):
    sizes = [10, 9]
    rng = np.random.default_rng(8)
    pos = (rng.random((50, 2)) * 7).astype(F)
    val = rng.normal(size=50).astype(F)
    x = rng.normal(size=90).astype(F)
    w = fi.Weights(model_2=1.0)
    from field_interpolation_amd import _capi

    def refused(f, code, field=x):
        for call in (lambda: f.point_residuals(field), lambda: f.robust_reweight(field), lambda: f.solve_robust(rounds=1)):
            with pytest.raises(fi.FiError) as e:
                call()
            assert e.value.code == code, e.value
            assert _capi.lib().fi_last_error()

    slab = fi.LatticeField(sizes, rank=0, nranks=2)                    # a slab context
    slab.add_field_constraints(w)
    slab.add_points(1.0, 1, 0.0, 1, pos, None, None, val)
    refused(slab, 5, x[: slab.num_owned])
    coo = fi.LatticeField(sizes)                                       # rows from add_rows_coo
    coo.add_field_constraints(w)
    coo.add_points(1.0, 1, 0.0, 1, pos, None, None, val)
    coo.add_rows_coo([0], [3], [1.0], [0.5])
    refused(coo, 5)
    assert coo.solve_cg(error_tolerance=1e-6) is not None              # the context is still usable
    lin = fi.LatticeField(sizes)                                       # the linear-interpolation gradient kernel
    lin.add_field_constraints(w)
    lin.add_points(1.0, 1, 1.0, 2, pos, rng.normal(size=(50, 2)).astype(F), None, None)
    refused(lin, 5)
    assert lin.solve_cg(error_tolerance=1e-6) is not None
    empty = fi.LatticeField(sizes)                                     # no points
    empty.add_field_constraints(w)
    refused(empty, 3)
    assert empty.point_count() == 0
    fresh = fi.LatticeField(sizes)                                     # no solution, and none given
    fresh.add_field_constraints(w)
    fresh.add_points(1.0, 1, 0.0, 1, pos, None, None, val)
    for call in (lambda: fresh.point_residuals(), lambda: fresh.robust_reweight()):
        with pytest.raises(fi.FiError) as e:
            call()
        assert e.value.code == 3 and _capi.lib().fi_last_error()
    fresh.solve_cg(error_tolerance=1e-6)
    assert np.all(fresh.point_residuals() >= 0)                        # ... and with one
    with pytest.raises(KeyError):
        fresh.robust_reweight(loss="l1")
