"""The numpy oracle of the k-nearest-point and normal-estimation contracts (tests/normals_reference.py) against independent
statements: knn at k = 1 against nearest_reference.nearest, the fixed-count Jacobi iteration against numpy.linalg.eigh, the
sign and degenerate rules by hand, and the normals of a noiseless sphere against the analytic ones.  No GPU."""
import numpy as np
import pytest

import nearest_reference as NR
import normals_reference as R

CLOUDS = ["random", "identical", "collinear", "cluster", "single", "outside", "grid ties"]


def _queries(rng, sizes, n, pad=5.0):
    D = len(sizes)
    return np.stack([rng.uniform(-pad, s - 1 + pad, n) for s in sizes], 1).astype(np.float32).reshape(n, D)


def _cloud(rng, kind, sizes, n=4000):
    D = len(sizes)
    if kind == "random":
        return _queries(rng, sizes, n, 2.0)
    if kind == "identical":
        return np.tile(np.float32(np.array(sizes) / 3.0), (n // 4, 1)).astype(np.float32)
    if kind == "collinear":
        t = rng.uniform(0, 1, n).astype(np.float32)
        return (np.outer(t, np.array(sizes, np.float32) - 1)).astype(np.float32)
    if kind == "cluster":
        return (np.float32(2.0) + rng.normal(scale=0.01, size=(n, D))).astype(np.float32)
    if kind == "single":
        return np.array([np.array(sizes, np.float32) / 2.0], np.float32)
    if kind == "outside":
        a = _queries(rng, sizes, n // 2, 40.0)
        b = (rng.uniform(-1, 1, size=(n // 2, D)) * 1e6).astype(np.float32)
        return np.concatenate([a, b])
    return rng.integers(0, 8, size=(n, D)).astype(np.float32)       # many exact ties


@pytest.mark.parametrize("kind", CLOUDS)
def test_knn_of_one_is_nearest(kind):
    sizes = [20, 18, 16]
    rng = np.random.default_rng(CLOUDS.index(kind))
    pos = _cloud(rng, kind, sizes, 1200)
    pos[::97, 1] = np.nan
    q = np.concatenate([_queries(rng, sizes, 500), pos[:100]])
    q[3, 0] = np.inf
    for md in (np.inf, 1.5):
        d, i = R.knn(pos, q, 3, 1, md)
        wd, wi = NR.nearest(pos, q, 3, md)
        assert np.array_equal(d[:, 0].view(np.uint32), wd.view(np.uint32)) and np.array_equal(i[:, 0], wi)


def test_knn_orders_pairs_and_pads():
    pts = np.array([[0, 0], [1, 0], [1, 0], [np.nan, 0], [0, 2], [-1, 0]], np.float32)
    d, i = R.knn(pts, np.array([[0, 0], [np.nan, 1]], np.float32), 2, 8)
    assert i[0].tolist() == [0, 1, 2, 5, 4, -1, -1, -1]          # equal s: ascending index; the NaN point never
    assert d[0].tolist()[:5] == [0, 1, 1, 1, 2] and np.all(np.isinf(d[0, 5:]))
    assert np.all(np.isnan(d[1])) and np.all(i[1] == -1)
    d, i = R.knn(pts, np.array([[0, 0]], np.float32), 2, 8, max_distance=1.0)
    assert i[0].tolist() == [0, 1, 2, 5, -1, -1, -1, -1] and np.all(np.isinf(d[0, 4:]))
    for k in (1, 3, 5):                                           # a smaller k is a prefix
        dk, ik = R.knn(pts, pts, 2, k)
        d8, i8 = R.knn(pts, pts, 2, 8)
        assert np.array_equal(ik, i8[:, :k]) and np.array_equal(dk.view(np.uint32), d8[:, :k].view(np.uint32))


def _sphere(rng, n, noise=0.0):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return (15.5 + 9.3 * v + rng.normal(scale=noise, size=(n, 3)) * (noise > 0)).astype(np.float32)


def _eigh_cloud(kind, rng):
    if kind == "sphere":
        return _sphere(rng, 4000), 3, 16
    if kind == "noisy sphere":
        return _sphere(rng, 4000, 0.2), 3, 16
    if kind == "integer grid":
        return rng.integers(0, 24, size=(4000, 3)).astype(np.float32), 3, 16
    if kind == "plane":
        p = rng.uniform(0, 30, size=(4000, 3)).astype(np.float32)
        p[:, 2] = (0.25 * p[:, 0] + 0.5 * p[:, 1]).astype(np.float32)
        return p, 3, 16
    a = rng.uniform(0, 2 * np.pi, 4000)
    return np.stack([20 + 12 * np.cos(a), 20 + 12 * np.sin(a)], 1).astype(np.float32), 2, 8


@pytest.mark.parametrize("kind", ["sphere", "noisy sphere", "integer grid", "plane", "circle 2-D"])
def test_six_jacobi_sweeps_agree_with_eigh(kind):
    rng = np.random.default_rng(42)
    pts, D, k = _eigh_cloud(kind, rng)
    _, idx = R.knn(pts, pts, D, k)
    _, A, m = R.covariances(pts, D, idx)
    assert np.all(m == k)
    nrm, _ = R.normals_of(A)
    lam, vec = np.linalg.eigh(A)                                  # ascending eigenvalues
    gap = (lam[:, 1] - lam[:, 0]) / np.maximum(lam[:, -1], np.finfo(np.float64).tiny)
    ok = gap >= 1e-6
    assert ok.mean() >= 0.9, ok.mean()
    n0 = vec[:, :, 0]
    if D == 3:
        sin = np.linalg.norm(np.cross(nrm, n0), axis=1)
    else:
        sin = np.abs(nrm[:, 0] * n0[:, 1] - nrm[:, 1] * n0[:, 0])
    worst = (sin * gap)[ok].max()
    print("%s: %.1f %% of the points checked, max sin(angle) x gap = %.3g" % (kind, 100 * ok.mean(), worst))
    assert worst <= 1e-13
    dlam, _ = R.jacobi(A)
    assert np.abs(np.sort(dlam, axis=1) - lam).max() <= 1e-12 * max(1.0, np.abs(lam).max())


def test_sign_rules():
    rng = np.random.default_rng(3)
    pts = _sphere(rng, 600)
    n0, v0 = R.estimate_normals(pts, 3, 12)
    big = np.argmax(np.abs(n0), axis=1)
    assert np.all(np.take_along_axis(n0, big[:, None], 1) > 0)    # canonical: the largest component is positive
    centre = np.float32(15.5)
    out = R.estimate_normals(pts, 3, 12, viewpoints=centre + 2 * (pts - centre))[0]
    assert np.all(np.sum(out * (pts - centre), axis=1) > 0)       # per-point viewpoints outside: outward
    inn = R.estimate_normals(pts, 3, 12, viewpoints=np.full((1, 3), centre))[0]
    assert np.array_equal(inn, -out)                              # one viewpoint at the centre: inward
    assert np.array_equal(np.abs(out), np.abs(n0))
    assert np.array_equal(R.estimate_normals(pts, 3, 12, directions=out)[0], out)
    assert np.array_equal(R.estimate_normals(pts, 3, 12, directions=-out)[0], -out)
    # w == 0 and a non-finite w keep the canonical sign
    g = np.zeros_like(pts)
    assert np.array_equal(R.estimate_normals(pts, 3, 12, directions=g)[0], n0)
    g[:] = np.nan
    assert np.array_equal(R.estimate_normals(pts, 3, 12, directions=g)[0], n0)
    assert np.array_equal(R.estimate_normals(pts, 3, 12, viewpoints=np.full((1, 3), -np.inf, np.float32))[0], n0)
    assert np.array_equal(R.estimate_normals(pts, 3, 12, viewpoints=pts)[0], n0)   # the viewpoint is the point: w == 0


def test_degenerate_outputs():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [np.nan, 0, 0], [50, 50, 50], [50, 51, 50]], np.float32)
    n, v = R.estimate_normals(pts, 3, 4, max_distance=2.0)
    assert np.array_equal(n[:4], np.tile(np.float32([0, 0, 1]), (4, 1)))   # a plane z = 0
    assert np.all(v[:4] == 0)
    assert np.all(n[4:] == 0) and np.all(np.isnan(v[4:]))         # non-finite; m = 2 < 3
    same = np.ones((5, 2), np.float32)                            # identical points: a zero matrix, the first column
    n, v = R.estimate_normals(same, 2, 4)
    assert np.array_equal(n, np.tile(np.float32([1, 0]), (5, 1))) and np.all(v == 0)
    with pytest.raises(ValueError):
        R.estimate_normals(pts[:, :1], 1, 4)
    with pytest.raises(ValueError):
        R.estimate_normals(pts, 3, 2)


# the oracle's own error on the fixture cloud of the test below, measured once: max 3.556 deg, mean 0.838 deg -- the
# curvature of a 16-point cap of this sphere, not rounding (numpy.linalg.eigh gives the same angles)
MEASURED_MAX = 3.556


def test_oracle_normals_of_a_noiseless_sphere():
    """4000 points on a sphere of radius 0.3 * 31 in a 32^3 lattice, k = 16, per-point viewpoints at centre + 2 (p - centre)"""
    rng = np.random.default_rng(2024)
    pts = _sphere(rng, 4000)
    centre = np.float32(15.5)
    n, var = R.estimate_normals(pts, 3, 16, viewpoints=centre + 2 * (pts - centre))
    want = (pts - centre).astype(np.float64)
    want /= np.linalg.norm(want, axis=1)[:, None]
    cos = np.sum(n.astype(np.float64) * want, axis=1)
    assert np.all(cos > 0)
    ang = np.degrees(np.arccos(np.clip(cos, -1, 1)))
    print("oracle on the sphere: max angle %.3f deg, mean %.3f deg" % (ang.max(), ang.mean()))
    assert ang.max() <= 1.5 * MEASURED_MAX
    assert np.all(var >= 0) and var.max() < 0.05                  # locally flat
