"""The numpy restatement of the robust fits (tests/robust_reference.py) held to the oracle: its residuals are the oracle's
rows applied to a field, its weight functions give the hand values of the contract, and its fp64 loop alone recovers the
truth from data with gross errors.  No GPU."""
import numpy as np
import pytest

import robust_reference as R
from oracle import fi_oracle

F = np.float32


def _edge_points(sizes, n, rng):
    """random points, and the cases where the row rules branch: negative coordinates above -1, the last lattice point,
    exact lattice positions, points outside"""
    gn = np.asarray(sizes, np.float64)
    D = len(sizes)
    p = rng.random((n, D)) * (gn - 1.0)
    p[0] = gn - 1.0                                  # the last lattice point
    p[1] = 0.0
    p[2:12] = np.floor(p[2:12])                      # exact lattice positions
    p[12:20, 0] = -rng.random(8) * 0.99              # above -1
    p[20:24] = -rng.random((4, D)) * 0.99
    p[24:28, -1] = gn[-1] - 1.0 + rng.random(4) * 0.9   # beyond the last point, inside the extended cells
    p[28:32, 0] = gn[0] + 3.0                        # outside
    p[32:34, -1] = -1.5
    p[34:40] = np.floor(p[34:40]) + 0.5              # where roundf has to decide
    return p.astype(F)


def _oracle_residuals(sizes, pos, nrm, val, vw, vk, gw, gk, x):
    """every point added on its own at unit point weight: the rows it gains are its rows; A x - b per row in fp64"""
    f = fi_oracle.LatticeField(sizes)
    spans = []
    for i in range(len(pos)):
        r0 = f.num_rows
        if nrm is None:
            f.add_value_constraint(pos[i], float(val[i]), float(vw))
        else:
            f.add_points(float(vw), vk, float(gw), gk, pos[i:i + 1], nrm[i:i + 1], None)
        spans.append((r0, f.num_rows))
    rows, cols, vals, rhs = f.get()
    e = -rhs.astype(np.float64)
    np.add.at(e, rows, vals.astype(np.float64) * x[cols])
    mag = np.abs(rhs.astype(np.float64))
    np.add.at(mag, rows, np.abs(vals.astype(np.float64) * x[cols]))
    r = np.array([np.sqrt(np.sum(e[a:b] ** 2)) if b > a else -1.0 for a, b in spans])
    smag = np.array([np.sqrt(np.sum(mag[a:b] ** 2)) for a, b in spans])
    return r, smag


CONFIGS = [(vk, gk) for vk in (R.VALUE_NEAREST, R.VALUE_LINEAR) for gk in (R.GRAD_NEAREST, R.GRAD_CELL_EDGES)] + [(R.VALUE_LINEAR, None)]


@pytest.mark.parametrize("sizes", [[33], [17, 13], [9, 8, 7]])
@pytest.mark.parametrize("vk,gk", CONFIGS)
def test_residuals_are_the_oracles_rows_applied_to_the_field(sizes, vk, gk):
    rng = np.random.default_rng(len(sizes) * 10 + vk * 3 + (gk or 0))
    D = len(sizes)
    n = 160
    pos = _edge_points(sizes, n, rng)
    x32 = rng.normal(size=int(np.prod(sizes))).astype(F)      # not a solution; exactly representable in both precisions
    x = x32.astype(np.float64)
    vw, gw = F(0.7), F(0.3)
    if gk is None:
        nrm, val = None, rng.normal(size=n).astype(F)
    else:
        nrm, val = rng.normal(size=(n, D)).astype(F), None
    want, smag = _oracle_residuals(sizes, pos, nrm, val, vw, vk, gw, gk if gk is not None else 0, x)
    b = R.batch(pos, nrm=nrm, val=val, vw=vw, vk=vk, gw=gw, gk=gk if gk is not None else R.GRAD_CELL_EDGES)
    got64 = R.residuals(sizes, [b], x, np.float64, rounded=False)
    assert np.array_equal(got64 < 0, want < 0)
    assert (want >= 0).sum() > n // 2 and (want < 0).sum() >= 4
    live = want >= 0
    assert np.all(np.abs(got64[live] - want[live]) <= 1e-12 * np.maximum(want[live], smag[live]))
    # fp32: a row is 2^D products, 2^D additions and one subtraction, each within 2^-24 of the running magnitude
    # S = sum |c x| + |b|: |e32 - e64| <= (2^(D+1) + 1) 2^-24 S.  r = sqrt(sum e^2) moves by at most sqrt(sum de^2); its own
    # D + 1 squares, D additions and the root (whose result is the rounding to float) add (2 D + 2) 2^-24 r.  1 % for the
    # second-order terms.
    got32 = R.residuals(sizes, [b], x32, np.float32)
    assert got32.dtype == F and np.array_equal(got32 < 0, want < 0)
    bound = 2.0 ** -24 * ((2 ** (D + 1) + 1) * smag + (2 * D + 2) * want) * 1.01
    err = np.abs(got32[live].astype(np.float64) - want[live])
    assert np.all(err <= bound[live]), (err / np.maximum(bound[live], 1e-300)).max()
    # the rounded fp64 residual is that residual rounded once
    assert np.array_equal(R.residuals(sizes, [b], x, np.float64)[live], got64[live].astype(F))


def test_zero_base_weight_and_prior_batches_take_no_part():
    sizes = [9, 8]
    rng = np.random.default_rng(5)
    pos = (rng.random((20, 2)) * 6).astype(F)
    pw = np.ones(20, F)
    pw[3] = 0.0
    x = rng.normal(size=72).astype(F)
    r = R.residuals(sizes, [R.batch(pos, val=np.zeros(20), pw=pw), R.batch(pos, val=np.zeros(20), prior=True)], x)
    assert len(r) == 20 and r[3] == -1 and np.all(np.delete(r, 3) >= 0)
    # the residual is measured at weight 1: other base weights do not change it
    r2 = R.residuals(sizes, [R.batch(pos, val=np.zeros(20), pw=pw * F(3.5))], x)
    assert np.array_equal(r, r2)


def test_omega_on_hand_values():
    two = F(2.0)
    below, above = np.nextafter(two, F(0)), np.nextafter(two, F(4))
    r = np.array([0.0, 2.0, below, above, 1e30, -1.0], F)
    s, c = F(1.0), 2.0        # s * c = 2 exactly: u = 0, 1, just below, just above, 5e29
    u_below, u_above = F(below / two), F(above / two)
    assert u_below < 1 < u_above
    h = R.omega(R.HUBER, r, s, c)
    assert list(h[:3]) == [1, 1, 1] and h[3] == F(1) / u_above and h[3] < 1 and h[4] == F(1) / F(F(1e30) / two) and h[5] == 1
    k = R.omega(R.CAUCHY, r, s, c)
    assert k[0] == 1 and k[1] == F(0.5) and k[2] == F(1) / (F(1) + u_below * u_below) and k[3] < F(0.5) and k[4] == 0 and k[5] == 1
    t = R.omega(R.TUKEY, r, s, c)
    tb = F(1) - u_below * u_below
    assert t[0] == 1 and t[1] == 0 and t[2] == tb * tb and t[2] > 0 and t[3] == 0 and t[4] == 0 and t[5] == 1
    for loss in (R.HUBER, R.CAUCHY, R.TUKEY):
        assert R.omega(loss, r, 0.0) is None                         # s = 0: the step changes nothing
        assert R.omega(loss, r, s, c).dtype == F
    # the defaults
    assert R.omega(R.HUBER, np.array([1.345 * 2], F), 1.0)[0] == F(1) / (F(2.69) / F(1.345))
    assert np.array_equal(R.point_weights([2.0, 3.0], [0.25, 0.0]), np.array([1.0, 0.0], F))


def test_scale_takes_the_lower_median():
    k = F(1.4826)
    assert R.scale([3.0]) == k * F(3)
    assert R.scale([5.0, 3.0]) == k * F(3)                            # M = 2: rank 0
    assert R.scale([5.0, 3.0, 4.0]) == k * F(4)                       # M = 3: rank 1
    assert R.scale([5.0, 3.0, 4.0, 9.0]) == k * F(4)                  # M = 4: rank 1
    assert R.scale([2.0, 2.0, 7.0, 2.0]) == k * F(2)                  # ties
    assert R.scale([7.0, -1.0, 2.0, -1.0, 7.0]) == k * F(7)           # points without rows do not count: M = 3
    assert R.scale([0.0, 0.0, 0.0, 1.0]) == 0 and R.scale([-1.0]) == 0 and R.scale([]) == 0
    assert R.scale([1.0]).dtype == F


CASES = [([24, 20, 16], 6000, 1.0), ([64, 64], 3000, 3.0)]


@pytest.mark.parametrize("sizes,npoints,model_2", CASES)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_reference_alone_beats_the_plain_fit(sizes, npoints, model_2, seed):
    b, bad = R.noisy_value_data(sizes, npoints, seed)
    assert 0.07 < bad.mean() < 0.13
    w = fi_oracle.Weights(model_2=model_2)
    want = R.truth_on_lattice(sizes)
    first = None
    for loss in (R.HUBER, R.CAUCHY, R.TUKEY):
        x, om, fields = R.irls(sizes, w, [b], loss=loss, rounds=5, first=first)
        assert len(fields) == 6
        first = fields[0]
        plain = R.rms(first, want)
        robust = R.rms(x, want)
        print("%s seed %d %s: plain %.4f robust %.4f ratio %.3f" % (sizes, seed, loss, plain, robust, robust / plain))
        assert robust <= 0.25 * plain, (loss, plain, robust)
        assert om[bad].mean() < 0.2 < 0.8 < om[~bad].mean()
