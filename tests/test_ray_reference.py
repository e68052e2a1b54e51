"""The numpy restatement of the ray contract (tests/ray_reference.py) against known answers, against the producers' inside
masks, against itself (tree-filtered equals brute force) and against an independent float64 Moeller-Trumbore.  No GPU."""
import numpy as np
import pytest

import ray_reference as R
from nearest_reference import lattice_points
from ray_cases import (BLOB_SIZES, CUBE_I, CUBE_V, SQUARE_I, SQUARE_V, F, axis_directions, mesh_of, same_bits, soup,
                       soup_rays)

INF = np.inf


def cast(v, i, o, d, **kw):
    return R.raycast(v, i, v.shape[1], np.asarray(o, F), np.asarray(d, F), **kw)


def count(v, i, o, d, **kw):
    return R.count_hits(v, i, v.shape[1], np.asarray(o, F), np.asarray(d, F), **kw)


# ---- the unit cube and the unit square: known answers ----------------------------------------------------------------------
@pytest.mark.parametrize("filtered", [False, True])
def test_cube_face_centres(filtered):
    o = [[-2, .5, .5]]
    for scale in (1, 2):
        d = [[scale, 0, 0]]
        t, j, b = cast(CUBE_V, CUBE_I, o, d, filtered=filtered)
        assert t[0] == 2 / scale and j[0] in (8, 9)
        t2, j2, _ = cast(CUBE_V, CUBE_I, o, d, t_min=np.nextafter(F(2 / scale), F(9)), filtered=filtered)
        assert t2[0] == 3 / scale and j2[0] in (10, 11)
        assert count(CUBE_V, CUBE_I, o, d, filtered=filtered)[0] == 2
    # (the face centre lies on the diagonal both triangles of a face share: one of them owns it)
    for a in range(3):
        for s in (1, -1):
            oo = np.full((1, 3), .5, F)
            oo[0, a] = -2 if s > 0 else 3
            dd = np.zeros((1, 3), F)
            dd[0, a] = s
            assert count(CUBE_V, CUBE_I, oo, dd, filtered=filtered)[0] == 2
            same_bits(cast(CUBE_V, CUBE_I, oo, dd, filtered=filtered)[0], F([2]))


@pytest.mark.parametrize("filtered", [False, True])
def test_cube_edges_and_corners_count_once(filtered):
    # through the edges x = y = 0 and x = y = 1; through the corners (0, 0, 0) and (1, 1, 1)
    for o, d in (([-1, -1, .5], [1, 1, 0]), ([-1, -1, -1], [1, 1, 1]), ([2, 2, .25], [-1, -1, 0]), ([2, 2, 2], [-.5, -.5, -.5]),
                 ([.5, -1, -1], [0, 1, 1]), ([-1, .5, 2], [1, 0, -1])):
        scale = 1 / max(abs(x) for x in d)
        assert count(CUBE_V, CUBE_I, [o], [d], t_max=1.5 * scale, filtered=filtered)[0] == 1, (o, d)
        assert count(CUBE_V, CUBE_I, [o], [d], filtered=filtered)[0] == 2, (o, d)
        t = cast(CUBE_V, CUBE_I, [o], [d], filtered=filtered)[0]
        assert t[0] == scale
    # grazing an edge or a corner from outside: both sheets or neither
    for o, d in (([-1, 1, .5], [1, -1, 0]), ([-1, 1, 0], [1, -1, 0]), ([-1, -1, 2], [1, 1, -1])):
        assert count(CUBE_V, CUBE_I, [o], [d], filtered=filtered)[0] % 2 == 0, (o, d)
    # 2-D: the square's corners
    for o, d in (([-1, -1], [1, 1]), ([2, 2], [-1, -1]), ([2, -1], [-1, 1])):
        assert count(SQUARE_V, SQUARE_I, [o], [d], t_max=1.5, filtered=filtered)[0] == 1
        assert count(SQUARE_V, SQUARE_I, [o], [d], filtered=filtered)[0] == 2
    t, j, b = cast(SQUARE_V, SQUARE_I, [[-2, .5]], [[1, 0]], filtered=filtered)
    assert t[0] == 2 and j[0] == 3 and b[0, 0] == .5
    t, j, _ = cast(SQUARE_V, SQUARE_I, [[-2, .5]], [[2, 0]], t_min=1.25, filtered=filtered)
    assert t[0] == 1.5 and j[0] == 1


@pytest.mark.parametrize("filtered", [False, True])
def test_ray_in_a_face_plane_misses_that_face(filtered):
    face = CUBE_I[:2]                                           # z = 0
    for o, d in (([-2, .5, 0], [1, 0, 0]), ([.5, .5, 0], [1, 1, 0]), ([.25, 3, 0], [0, -1, 0])):
        t, j, _ = cast(CUBE_V, face, [o], [d], t_min=-INF, filtered=filtered)
        assert np.isposinf(t[0]) and j[0] == -1
        j = cast(CUBE_V, CUBE_I, [o], [d], filtered=filtered)[1]
        assert j[0] not in (0, 1)
    # a 2-D ray along a segment does not cross it
    assert count(SQUARE_V, SQUARE_I[:1], [[-1, 0]], [[1, 0]], filtered=filtered)[0] == 0


@pytest.mark.parametrize("filtered", [False, True])
def test_window_ties_limit_and_bad_rays(filtered):
    o, d = [[-2, .5, .5]], [[1, 0, 0]]
    up, down = np.nextafter(F(2), F(9)), np.nextafter(F(3), F(0))
    for lo, hi, n in ((2, 2, 1), (2, 3, 2), (3, 3, 1), (up, down, 0), (up, 3, 1), (2, down, 1), (-INF, INF, 2), (3, INF, 1),
                      (-INF, 2, 1), (4, INF, 0)):
        assert count(CUBE_V, CUBE_I, o, d, t_min=lo, t_max=hi, filtered=filtered)[0] == n, (lo, hi)
        t, j, _ = cast(CUBE_V, CUBE_I, o, d, t_min=lo, t_max=hi, filtered=filtered)
        assert (j[0] >= 0) == (n > 0) and (np.isposinf(t[0]) if n == 0 else t[0] == max(2, np.ceil(lo)))
    # the same triangles twice: the smaller index wins the tie
    twice = np.concatenate([CUBE_I[::-1], CUBE_I])
    t, j, _ = cast(CUBE_V, twice, o, d, filtered=filtered)
    t1, j1, _ = cast(CUBE_V, CUBE_I, o, d, filtered=filtered)
    assert t[0] == 2 and j[0] == 11 - j1[0]
    assert count(CUBE_V, twice, o, d, filtered=filtered)[0] == 4
    for limit, n in ((1, 1), (2, 2), (3, 3), (4, 4), (5, 4)):
        assert count(CUBE_V, twice, o, d, limit=limit, filtered=filtered)[0] == n
    # rays that are no rays
    O = np.array([[-2, .5, .5]] * 5, F)
    Dr = np.array([[1, 0, 0]] * 5, F)
    O[1, 1], O[2, 0], Dr[3], Dr[4, 2] = np.nan, np.inf, 0, -np.inf
    t, j, b = cast(CUBE_V, CUBE_I, O, Dr, filtered=filtered)
    assert t[0] == 2 and np.all(np.isnan(t[1:])) and np.all(j[1:] == -1) and np.all(np.isnan(b[1:]))
    assert list(count(CUBE_V, CUBE_I, O, Dr, filtered=filtered)) == [2, 0, 0, 0, 0]
    for lo, hi in ((1, 0), (np.nan, 1), (0, np.nan)):
        with pytest.raises(R.Invalid):
            cast(CUBE_V, CUBE_I, o, d, t_min=lo, t_max=hi)
    with pytest.raises(R.Invalid):
        count(CUBE_V, CUBE_I, o, d, limit=0)
    # no primitives, no rays
    assert np.isposinf(cast(CUBE_V, CUBE_I[:0], o, d)[0][0])
    assert cast(CUBE_V, CUBE_I, np.zeros((0, 3)), np.zeros((0, 3)))[0].shape == (0,)


# ---- parity against the producers' inside masks -------------------------------------------------------------------------------
def parity_directions(ndim, seed=3):
    diag = {3: [[1, 1, 0], [0, 1, -1], [1, -1, 1]], 2: [[1, 1], [1, -1], [-1, 2]]}[ndim]
    rnd = np.random.default_rng(seed).normal(size=(3, ndim))
    return np.concatenate([axis_directions(ndim), np.array(diag, F), rnd.astype(F)])


@pytest.mark.parametrize("method", ["iso", "dual"])
@pytest.mark.parametrize("sizes", [BLOB_SIZES, BLOB_SIZES[:2]])
def test_parity_equals_the_inside_mask_of_a_closed_mesh(sizes, method):
    v, i, inside, _f, _iso = mesh_of("blob", sizes, method)
    assert inside.any() and not inside.all()
    pts = lattice_points(sizes)
    for d in parity_directions(len(sizes)):
        got = R.contains(v, i, len(sizes), pts, d)
        assert np.array_equal(got, inside), (d, np.flatnonzero(got != inside)[:10])
    assert np.array_equal(R.contains(v, i, len(sizes), pts), inside)


@pytest.mark.parametrize("method", ["iso", "dual"])
@pytest.mark.parametrize("sizes", [[9, 7, 8], [7, 5, 6]])
def test_parity_along_the_rows_of_an_open_mesh(sizes, method):
    v, i, inside, _f, _iso = mesh_of("smooth", sizes, method)
    pts = lattice_points(sizes)
    c = pts.astype(np.int64)
    lin = lambda p: p[:, 0] + sizes[0] * (p[:, 1] + sizes[1] * p[:, 2])  # noqa: E731
    for d in axis_directions(3):
        a = int(np.flatnonzero(d)[0])
        others = [b for b in range(3) if b != a]
        rows = np.all([(c[:, b] > 0) & (c[:, b] < sizes[b] - 1) for b in others], axis=0)
        end = c.copy()
        end[:, a] = sizes[a] - 1 if d[a] > 0 else 0
        want = inside ^ inside[lin(end)]
        got = R.contains(v, i, 3, pts, d)
        assert np.array_equal(got[rows], want[rows]), (d, np.flatnonzero((got != want) & rows)[:10])


# ---- tree-filtered against brute force ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0.0, 4096.0])
@pytest.mark.parametrize("n", [1, 8, 9, 500])
@pytest.mark.parametrize("ndim", [2, 3])
def test_filtered_equals_brute_force(ndim, n, shift):
    for flat, bad in ((False, False), (True, False), (True, True)):
        v, i = soup(n, 100 + n, ndim, shift, flat, bad)
        o, d = soup_rays(600, 7 + n, ndim, shift, flat)
        for lo, hi in ((0.0, INF), (-INF, INF), (0.5, 6.0)):
            a = R.raycast(v, i, ndim, o, d, lo, hi, filtered=False)
            b = R.raycast(v, i, ndim, o, d, lo, hi, filtered=True)
            same_bits(b[0], a[0])
            assert np.array_equal(a[1], b[1])
            same_bits(b[2], a[2])
            ca = R.count_hits(v, i, ndim, o, d, lo, hi, filtered=False)
            assert np.array_equal(ca, R.count_hits(v, i, ndim, o, d, lo, hi, filtered=True))
            if n >= 8 and not shift:
                assert ca.max() >= 1 and (a[1] >= 0).sum() >= 5


# ---- an independent float64 Moeller-Trumbore ------------------------------------------------------------------------------------
def moller_trumbore(P, o, d):
    """(t, u, v) float64 of rays o, d (m, 3) against triangles P (k, 3, 3), (m, k) each; NaN where parallel"""
    e1, e2 = P[None, :, 1] - P[None, :, 0], P[None, :, 2] - P[None, :, 0]
    h = np.cross(d[:, None, :], e2)
    a = np.sum(e1 * h, axis=2)
    with np.errstate(all="ignore"):
        f = 1.0 / a
        s = o[:, None, :] - P[None, :, 0]
        u = f * np.sum(s * h, axis=2)
        q = np.cross(s, e1)
        v = f * np.sum(d[:, None, :] * q, axis=2)
        t = f * np.sum(e2 * q, axis=2)
    return t, u, v


# the worst |t - t64| observed on the rays kept (seed 5, 4096 rays, 24^3 smooth mesh) is 8.41e-6, at t up to ~60 where one
# fp32 ulp of t is 3.8e-6 and the fp32 projection of a vertex carries a few ulps of its coordinates: the tolerance is 4 x that
MT_TOLERANCE = 4 * 8.41e-6


def test_against_float64_moller_trumbore():
    """Random rays against the 24^3 mesh: on every ray that float64 does not call a close call (barycentrics within 1e-4
    of an edge, or its two nearest hits within 1e-4 in t), the primitive is the same and t agrees within MT_TOLERANCE.
    Measured here: 0.20 % of the rays excluded, worst |t - t64| = 8.41e-6."""
    sizes = [24, 24, 24]
    v, i, _inside, _f, _iso = mesh_of("smooth", sizes, "iso")
    rng = np.random.default_rng(5)
    m = 4096
    o = rng.uniform(-4, 28, (m, 3)).astype(F)
    target = rng.uniform(4, 20, (m, 3))
    d = (target - o).astype(F)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2, (m, 1))).astype(F)
    P = v[i].astype(np.float64)
    keep = np.ones(m, bool)
    t64 = np.full(m, np.inf)
    j64 = np.full(m, -1, np.int64)
    for b in range(0, m, 256):
        t, u, w = moller_trumbore(P, o[b: b + 256].astype(np.float64), d[b: b + 256].astype(np.float64))
        with np.errstate(invalid="ignore"):
            e = 1e-4
            hit = (u >= 0) & (w >= 0) & (u + w <= 1) & (t >= 0)
            close = (u >= -e) & (w >= -e) & (u + w <= 1 + e) & (t >= -e) & ~((u >= e) & (w >= e) & (u + w <= 1 - e) & (t >= e))
        tt = np.where(hit, t, np.inf)
        order = np.argsort(tt, axis=1)
        r = np.arange(tt.shape[0])
        first, second = tt[r, order[:, 0]], tt[r, order[:, 1]]
        t64[b: b + 256] = first
        j64[b: b + 256] = np.where(np.isfinite(first), order[:, 0], -1)
        with np.errstate(invalid="ignore"):
            keep[b: b + 256] = ~close.any(axis=1) & ~(second - first < 1e-4)
    excluded = 1 - keep.mean()
    print("excluded share %.4f, hits %d" % (excluded, (j64 >= 0).sum()))
    assert excluded <= 0.02
    assert (j64[keep] >= 0).sum() > m // 2
    t, j, _b = R.raycast(v, i, 3, o, d)
    assert np.array_equal(j[keep], j64[keep])
    got = np.where(j >= 0, t, np.inf)[keep]
    with np.errstate(invalid="ignore"):
        diff = np.where(np.isfinite(t64[keep]), np.abs(got - t64[keep]), 0)
    print("worst |t - t64| = %.3g" % diff.max())
    assert diff.max() <= MT_TOLERANCE
