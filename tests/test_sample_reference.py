"""The point-query oracle itself (tests/sample_reference.py), on the CPU: its linear weights are the reference's value-row
coefficients bit for bit, linear mode reproduces multilinear functions and cubic mode quadratics, lattice values come back
exactly, and gradients agree with analytic ones and with central differences of the sampler."""
import numpy as np
import pytest

import sample_reference as R
from oracle import fi_oracle


def _grid(sizes):
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sizes[::-1]], indexing="ij")
    return [g[len(sizes) - 1 - d].reshape(-1) for d in range(len(sizes))]  # coordinate d of every point, x fastest


@pytest.mark.parametrize("sizes", [[9], [7, 6], [5, 6, 7]])
def test_linear_weights_are_the_value_row_coefficients(sizes):
    rng = np.random.default_rng(len(sizes))
    D = len(sizes)
    pos = (rng.uniform(0, 1, size=(200, D)) * (np.array(sizes) - 1.0001)).astype(np.float32)
    pos[:20] = np.floor(pos[:20])                       # integer coordinates too
    assert np.all(pos < np.array(sizes, np.float32) - 1)  # every corner inside
    inside, c, t = R.locate(sizes, pos)
    assert inside.all()
    w, _ = R.linear_weights(t)
    strides = np.cumprod([1] + sizes[:-1])
    for k, p in enumerate(pos):
        f = fi_oracle.LatticeField(sizes)
        assert f.add_value_constraint(p, 1.0, 1.0)
        rows, cols, vals, rhs = f.get()
        want_cols = [int(sum(strides[d] * (c[k, d] + ((i >> d) & 1)) for d in range(D))) for i in range(1 << D)]
        assert list(cols) == want_cols
        got = np.array([w[i][k] for i in range(1 << D)], np.float32)
        assert np.array_equal(got.view(np.uint32), vals.view(np.uint32))


def _poly_field(sizes, coef, cubic):
    x = _grid(sizes)
    D = len(sizes)
    f = np.full(x[0].shape, coef[0])
    grad = []
    for d in range(D):
        f += coef[1 + d] * x[d]
    if D > 1:  # a multilinear cross term
        f += coef[4] * x[0] * x[1]
    if cubic:  # quadratic terms
        for d in range(D):
            f += coef[5 + d] * x[d] ** 2
    def value(p):
        v = coef[0] + sum(coef[1 + d] * p[:, d] for d in range(D))
        if D > 1:
            v = v + coef[4] * p[:, 0] * p[:, 1]
        if cubic:
            v = v + sum(coef[5 + d] * p[:, d] ** 2 for d in range(D))
        return v
    def gradient(p):
        g = np.stack([np.full(len(p), coef[1 + d]) for d in range(D)], axis=1)
        if D > 1:
            g[:, 0] += coef[4] * p[:, 1]
            g[:, 1] += coef[4] * p[:, 0]
        if cubic:
            for d in range(D):
                g[:, d] += 2 * coef[5 + d] * p[:, d]
        return g
    return f, value, gradient


@pytest.mark.parametrize("cubic", [False, True])
@pytest.mark.parametrize("sizes", [[11], [9, 8], [7, 8, 9]])
def test_reproduces_polynomials(sizes, cubic):
    rng = np.random.default_rng(3)
    D = len(sizes)
    coef = rng.uniform(-1, 1, size=8)
    f, value, gradient = _poly_field(sizes, coef, cubic)
    lo = 1.0 if cubic else 0.0                       # cubic: no clamped index (cells 1 .. n - 3)
    hi = np.array(sizes) - (2.0 if cubic else 1.0)
    pos = (lo + rng.uniform(0, 1, size=(300, D)) * (hi - lo)).astype(np.float32)
    p64 = pos.astype(np.float64)
    for dtype, tol in ((np.float32, 2e-5), (np.float64, 1e-6)):
        v, g = R.sample(f, sizes, pos, cubic=cubic, gradients=True, dtype=dtype)
        scale = np.abs(f).max()
        assert np.abs(v - value(p64)).max() <= tol * scale
        assert np.abs(g - gradient(p64)).max() <= tol * scale * 4


@pytest.mark.parametrize("cubic", [False, True])
@pytest.mark.parametrize("sizes", [[9], [7, 6], [5, 6, 7]])
def test_lattice_values_come_back_exactly(sizes, cubic):
    rng = np.random.default_rng(5)
    f = rng.normal(size=int(np.prod(sizes))).astype(np.float32)
    x = np.stack(_grid(sizes), axis=1)
    below = np.all(x < np.array(sizes) - 1, axis=1)       # below the upper face: t = 0 in every axis
    v = R.sample(f, sizes, x[below].astype(np.float32), cubic=cubic)
    assert np.array_equal(v.view(np.uint32), f[below].view(np.uint32))
    # on the upper face the last cell is used with t = 1: the value is still the lattice value (to rounding)
    v = R.sample(f, sizes, x.astype(np.float32), cubic=cubic)
    assert np.allclose(v, f, rtol=0, atol=1e-6)


@pytest.mark.parametrize("cubic", [False, True])
@pytest.mark.parametrize("sizes", [[13], [9, 8], [7, 8, 6]])
def test_gradients_are_central_differences(sizes, cubic):
    rng = np.random.default_rng(11)
    D = len(sizes)
    x = _grid(sizes)
    f = np.cos(sum(0.4 * (d + 1) * x[d] for d in range(D))).astype(np.float32)
    pos = (rng.uniform(0.1, 0.9, size=(200, D)) * (np.array(sizes) - 1)).astype(np.float32)
    # keep every coordinate away from a cell boundary (the linear gradient jumps there)
    frac = pos - np.floor(pos)
    pos = np.where((frac < 0.01) | (frac > 0.99), np.floor(pos) + 0.5, pos).astype(np.float32)
    _, g = R.sample(f, sizes, pos, cubic=cubic, gradients=True, dtype=np.float64)
    h = 1e-3
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        # the fp64 path on float64 positions: the widened position is the point itself
        vp = _sample64(f, sizes, pos.astype(np.float64) + e, cubic)
        vm = _sample64(f, sizes, pos.astype(np.float64) - e, cubic)
        assert np.abs((vp - vm) / (2 * h) - g[:, d]).max() <= 1e-4


def _sample64(f, sizes, p, cubic):
    """the fp64 sampler at float64 positions (the oracle's internals, without the fp32 position and output roundings)"""
    c = np.minimum(np.floor(p).astype(np.int64), np.array(sizes) - 2)
    t = p - c
    v, _ = (R._cubic if cubic else R._linear)(f.astype(np.float64), sizes, c, t, False)
    return v


def test_outside_points_and_fill():
    sizes = [5, 4]
    f = np.arange(20, dtype=np.float32)
    pos = np.array([[-0.0, 0.0], [4.0, 3.0], [4.0001, 1.0], [-1e-7, 1.0], [np.nan, 1.0], [1.0, np.inf]], np.float32)
    v, g = R.sample(f, sizes, pos, gradients=True, fill=-7.0)
    assert v[0] == 0.0 and v[1] == 19.0
    assert np.all(v[2:] == -7.0) and np.all(g[2:] == -7.0)
    assert np.array_equal(g[1], [1.0, 5.0])
