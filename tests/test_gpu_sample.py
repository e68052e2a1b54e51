"""Point queries on the device (fi_sample.hip through fi_sample / fi_sample_field) against the numpy oracle of the contract
(tests/sample_reference.py), bit for bit: 1-, 2- and 3-D, odd sizes, linear and cubic, with and without gradients, edge
positions, bad arguments, solved fp32 and fp64 fields, and the lattice points of fi_upscale_field."""
import ctypes as C

import numpy as np
import pytest

import sample_reference as R
from util import sphere_points

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _same(got, want):
    """bit-equal, NaN payloads aside (a NaN field value may propagate with another payload)"""
    got = np.ascontiguousarray(got, np.float32).reshape(-1)
    want = np.ascontiguousarray(want, np.float32).reshape(-1)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    bad = np.flatnonzero(got.view(np.uint32)[~nan] != want.view(np.uint32)[~nan])
    assert bad.size == 0, (bad[:5], got[~nan][bad[:5]], want[~nan][bad[:5]])


def _check(fi, f, sizes, pos, cubic, gradients, fill=float("nan")):
    got = fi.sample_field(f, sizes, pos, gradients=gradients, cubic=cubic, fill=fill)
    want = R.sample(f, sizes, pos, cubic=cubic, gradients=gradients, fill=fill)
    if gradients:
        _same(got[0], want[0])
        _same(got[1], want[1])
        assert got[1].shape == (len(pos), len(sizes))
    else:
        _same(got, want)
    return got


def _edge_positions(rng, sizes, n):
    """random points over the lattice and a little beyond it, plus integer coordinates, the upper face, -0.0, just
    outside, NaN and inf"""
    D = len(sizes)
    hi = np.array(sizes, np.float32) - 1
    p = (rng.uniform(-0.05, 1.05, size=(n, D)) * hi).astype(np.float32)
    p[: n // 8] = np.round(p[: n // 8])                                         # integer coordinates
    k = n // 8
    p[k: k + 8] = hi                                                            # the upper corner
    p[k + 8: k + 16, 0] = hi[0]                                                 # the upper face of x
    p[k + 16: k + 24, D - 1] = hi[D - 1]                                        # ... and of the slowest axis
    p[k + 24: k + 32, 0] = -0.0
    p[k + 32, 0] = np.nextafter(np.float32(0), np.float32(-1))                  # just outside
    p[k + 33, D - 1] = np.nextafter(hi[D - 1], np.float32(np.inf))
    p[k + 34, 0] = np.nan
    p[k + 35, D - 1] = np.inf
    p[k + 36, 0] = -np.inf
    p[k + 37] = np.nextafter(hi, np.float32(0))                                 # just inside the upper corner
    return p


SIZES = [[7], [2], [9, 5], [2, 2], [13, 11, 7], [5, 2, 3], [17, 9, 12]]


@pytest.mark.parametrize("gradients", [False, True])
@pytest.mark.parametrize("cubic", [False, True])
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_matches_the_oracle(fi, sizes, cubic, gradients):
    rng = np.random.default_rng(sum(sizes) * 4 + 2 * cubic + gradients)
    f = rng.normal(size=int(np.prod(sizes))).astype(np.float32)
    _check(fi, f, sizes, _edge_positions(rng, sizes, 3000), cubic, gradients)


@pytest.mark.parametrize("cubic", [False, True])
def test_fill_and_non_finite_field_values(fi, cubic):
    sizes = [6, 5, 4]
    rng = np.random.default_rng(9)
    f = rng.normal(size=120).astype(np.float32)
    f[17] = np.inf
    f[60] = np.nan
    pos = _edge_positions(rng, sizes, 800)
    for fill in (-0.0, 5.0, float("nan")):
        _check(fi, f, sizes, pos, cubic, True, fill=fill)


def test_no_points(fi):
    f = np.zeros(12, np.float32)
    v, g = fi.sample_field(f, [4, 3], np.zeros((0, 2), np.float32), gradients=True)
    assert v.shape == (0,) and g.shape == (0, 2)


def test_bad_arguments(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    f = np.zeros(12, np.float32)
    sz = (C.c_int * 2)(4, 3)
    pos = np.ones((5, 2), np.float32)
    val = np.empty(5, np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    nan = float("nan")
    assert L.fi_sample_field(p(f), 2, sz, 5, p(pos), 0, nan, p(val), None, 0) == 0
    assert L.fi_sample_field(p(f), 2, sz, 5, p(pos), 2, nan, p(val), None, 0) == 1     # bad mode
    assert L.fi_sample_field(p(f), 2, sz, 5, p(pos), -1, nan, p(val), None, 0) == 1
    assert L.fi_sample_field(p(f), 2, sz, -1, p(pos), 0, nan, p(val), None, 0) == 1    # n < 0
    assert L.fi_sample_field(p(f), 2, sz, 5, None, 0, nan, p(val), None, 0) == 1       # NULL positions
    assert L.fi_sample_field(p(f), 2, sz, 5, p(pos), 0, nan, None, None, 0) == 1       # NULL values
    assert L.fi_sample_field(None, 2, sz, 5, p(pos), 0, nan, p(val), None, 0) == 1     # NULL field
    assert L.fi_sample_field(p(f), 2, None, 5, p(pos), 0, nan, p(val), None, 0) == 1   # NULL sizes
    assert L.fi_sample_field(p(f), 2, sz, 5, p(pos), 0, nan, p(val), None, 7) == 1     # bad memory kind
    assert L.fi_sample_field(p(f), 4, sz, 5, p(pos), 0, nan, p(val), None, 0) == 1     # ndim
    assert L.fi_sample_field(p(f), 2, (C.c_int * 2)(12, 1), 5, p(pos), 0, nan, p(val), None, 0) == 1  # a size < 2
    assert L.fi_sample_field(p(f), 1, (C.c_int * 1)(1), 5, p(pos), 0, nan, p(val), None, 0) == 1
    assert L.fi_sample_field(p(f), 2, sz, 0, p(pos), 1, nan, p(val), None, 0) == 0     # n = 0
    with pytest.raises(fi.FiError) as e:
        fi.sample_field(f, [12, 1], pos[:, :2])
    assert e.value.code == 1
    with pytest.raises(ValueError):
        fi.sample_field(f, [4, 3], np.ones(5, np.float32))
    # a context: no solution yet, bad arguments
    ctx = fi.LatticeField([4, 3])
    with pytest.raises(fi.FiError) as e:
        ctx.sample(pos)
    assert e.value.code == 3                                                              # FI_ERR_STATE
    assert L.fi_sample(ctx._h, p(f), 5, p(pos), 3, nan, p(val), None, 0) == 1
    assert L.fi_sample(ctx._h, p(f), -2, p(pos), 0, nan, p(val), None, 0) == 1
    assert L.fi_sample(ctx._h, p(f), 5, None, 0, nan, p(val), None, 0) == 1
    assert L.fi_sample(ctx._h, p(f), 5, p(pos), 0, nan, None, None, 0) == 1
    assert L.fi_sample(None, p(f), 5, p(pos), 0, nan, p(val), None, 0) == 1
    _same(ctx.sample(pos, f), R.sample(f, [4, 3], pos))                                  # owned values passed in
    thin = fi.LatticeField([5, 1])
    with pytest.raises(fi.FiError) as e:
        thin.sample(pos, np.zeros(5, np.float32))
    assert e.value.code == 1


def _solved(fi, sizes, dtype):
    rng = np.random.default_rng(len(sizes))
    pos, nrm = sphere_points(rng, sizes, 1500)
    f = fi.sdf_from_points(sizes, fi.Weights(), pos, nrm, dtype=dtype)
    x, it, rel = f.solve_cg(None, 0, 1e-6)
    return f, x, pos, nrm


@pytest.mark.parametrize("sizes", [[40, 36, 30], [97, 83]], ids=["3d", "2d"])
def test_residuals_at_the_data_points(fi, sizes):
    f, x, pos, nrm = _solved(fi, sizes, "f32")
    for cubic in (False, True):
        v, g = f.sample(pos, gradients=True, cubic=cubic)
        want_v, want_g = R.sample(x, sizes, pos, cubic=cubic, gradients=True)
        _same(v, want_v)
        _same(g, want_g)
        # an SDF fit: f(p_i) ~ 0 and grad f(p_i) along n_i
        assert np.median(np.abs(v)) < 0.3
        cos = np.sum(g * nrm, axis=1) / np.linalg.norm(g, axis=1)
        assert np.median(cos) > 0.9
    # the solution passed back in gives the same results
    _same(f.sample(pos, x, cubic=True), R.sample(x, sizes, pos, cubic=True))


@pytest.mark.parametrize("sizes", [[34, 30, 26], [71, 64]], ids=["3d", "2d"])
def test_f64_solution_in_place(fi, sizes):
    f, x, pos, nrm = _solved(fi, sizes, "f64")
    x64 = f.solution_f64()
    rng = np.random.default_rng(2)
    q = np.concatenate([pos, _edge_positions(rng, sizes, 500)])
    for cubic in (False, True):
        v, g = f.sample(q, gradients=True, cubic=cubic)
        want_v, want_g = R.sample(x64, sizes, q, cubic=cubic, gradients=True, dtype=np.float64)
        _same(v, want_v)
        _same(g, want_g)
        # fp32 values passed in are sampled in fp32
        _same(f.sample(q, x, cubic=cubic), R.sample(x, sizes, q, cubic=cubic))


UPSCALE = [([5, 6, 7], [13, 17, 19]), ([7, 9], [23, 31]), ([11], [37]), ([6, 5, 4], [9, 7, 11])]


@pytest.mark.parametrize("small,large", UPSCALE, ids=lambda s: "x".join(map(str, s)))
def test_linear_agrees_with_upscale_field(fi, small, large):
    rng = np.random.default_rng(sum(small))
    f = rng.uniform(1, 2, int(np.prod(small))).astype(np.float32)   # one sign: no cancellation in either sum
    up = fi.upscale_field(f, small, large)
    D = len(small)
    F = np.float32
    axes = [np.arange(large[d]).astype(F) * (F(small[d]) - F(1)) / (F(large[d]) - F(1)) for d in range(D)]
    mesh = np.meshgrid(*axes[::-1], indexing="ij")
    pos = np.stack([mesh[D - 1 - d].reshape(-1) for d in range(D)], axis=1).astype(F)   # the large lattice's points, x fastest
    v = fi.sample_field(f, small, pos)
    _same(v, R.sample(f, small, pos))
    # upscale_field divides by its weight sum, so the two agree to rounding only
    ulps = np.abs(v.astype(np.float64) - up) / np.spacing(np.maximum(np.abs(v), np.abs(up)))
    assert ulps.max() <= 2, ulps.max()
