"""The numpy definition of the moving-least-squares projection (tests/mls_reference.py) held to known answers: points on a
plane stay, a noisy sphere loses its noise under the quadric and shrinks under the plane, degenerate neighbourhoods are
refused the quadric, the Cholesky pivots sit where DESIGN.md 4.25 records them, a noisy circle's band gets thinner.  No GPU.
The figures in the comments are this file's own, measured with the definition."""
import numpy as np
import pytest

import mls_reference as M
import normals_reference as R

R0, SIGMA = 10.0, 0.05


@pytest.fixture(scope="module")
def sphere():
    """3 000 points of a sphere of radius 10 with radial noise 0.05, and their true normals"""
    rng = np.random.default_rng(0)
    d = rng.normal(size=(3000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = R0 + rng.normal(scale=SIGMA, size=3000)
    return (d * r[:, None]).astype(np.float32), d


@pytest.fixture(scope="module")
def fits(sphere):
    """the plane and the quadric at k = 32, radius 3: computed once, read by the tests below"""
    P, _ = sphere
    return {deg: M.project(P, 3, None, 32, 3.0, deg, details=True) for deg in (1, 2)}


def _radial(pos):
    return np.linalg.norm(pos.astype(np.float64), axis=1) - R0


def _angle_rms(nrm, d):
    c = np.clip(np.abs((nrm.astype(np.float64) * d).sum(1)), 0.0, 1.0)
    return np.sqrt(np.mean(np.degrees(np.arccos(c)) ** 2))


def test_points_on_a_plane_stay_where_they_are():
    rng = np.random.default_rng(1)
    uv = rng.uniform(0, 20, size=(1500, 2))
    # z = 3 + x / 4 + y / 2: every coordinate a float32 with bits to spare, so the points lie on the plane to ~1 ulp
    P = np.stack([uv[:, 0], uv[:, 1], 3.0 + 0.25 * uv[:, 0] + 0.5 * uv[:, 1]], 1).astype(np.float32)
    n_true = np.array([-0.25, -0.5, 1.0]) / np.linalg.norm([-0.25, -0.5, 1.0])
    for deg in (1, 2):
        pos, nrm, cur, order = M.project(P, 3, None, 32, 3.0, deg)
        assert set(np.unique(order)) <= {1, 2} and (deg == 1) == bool(np.all(order == 1))
        ulp = np.spacing(np.abs(P).max(axis=1))
        print("plane: degree %d, moved at most %.3g ulp, |curvature| <= %.3g" % (deg, (np.abs(pos - P).max(1) / ulp).max(),
                                                                                 np.abs(cur).max()))
        assert np.all(np.abs(pos - P).max(axis=1) <= 4 * ulp)       # fp32 rounding of the inputs and of the output
        assert np.abs(cur).max() <= 1e-5                            # the inputs' rounding, 1e-7 relative, over (h = 3)^2
        assert np.all(np.abs(np.abs(nrm.astype(np.float64) @ n_true) - 1.0) <= 1e-6)


def test_the_quadric_removes_noise_and_the_plane_shrinks_the_sphere(sphere, fits):
    P, d = sphere
    rms_in = np.sqrt(np.mean(_radial(P) ** 2))
    r1, r2 = _radial(fits[1][0]), _radial(fits[2][0])
    rms1, rms2 = np.sqrt(np.mean(r1 ** 2)), np.sqrt(np.mean(r2 ** 2))
    curv = np.abs(fits[2][2].astype(np.float64)).mean()
    print("sphere: input rms %.4f; plane rms %.4f bias %.4f angle %.2f deg; quadric rms %.4f bias %.4f angle %.2f deg, "
          "mean |curvature| %.4f" % (rms_in, rms1, r1.mean(), _angle_rms(fits[1][1], d), rms2, r2.mean(),
                                     _angle_rms(fits[2][1], d), curv))
    # measured: input 0.0498; plane 0.0713, bias -0.0696, 1.24 deg; quadric 0.0187 (0.38 x), bias -0.0001, 0.90 deg; 0.1010
    assert np.all(fits[1][3] == 1) and np.all(fits[2][3] == 2)
    assert rms2 <= 0.5 * rms_in
    assert abs(r2.mean()) <= 0.005
    assert r1.mean() < -0.05
    assert abs(curv - 1.0 / R0) <= 0.05 / R0
    assert _angle_rms(fits[2][1], d) < _angle_rms(fits[1][1], d) < 2.0
    # the curvature's sign: the canonical normal points outward on the half where its largest component does, and there the
    # sphere bends away from it
    outward = (fits[2][1].astype(np.float64) * d).sum(1) > 0
    assert np.all(fits[2][2][outward] < 0) and np.all(fits[2][2][~outward] > 0)


def test_too_few_points_for_six_coefficients_amplify_noise(sphere):
    # what the documentation warns of: at k = 16, radius 1.5 the quadric is worse than the plane (measured 0.0328 / 0.0273)
    P, _ = sphere
    rms = {deg: np.sqrt(np.mean(_radial(M.project(P, 3, None, 16, 1.5, deg)[0]) ** 2)) for deg in (1, 2)}
    print("sphere, k = 16, radius 1.5: plane rms %.4f, quadric rms %.4f" % (rms[1], rms[2]))
    assert rms[2] > rms[1]


def _degenerate():
    """(name, cloud, radius): neighbourhoods that do not determine a quadric"""
    rng = np.random.default_rng(2)
    t = rng.uniform(0, 1, 1000).astype(np.float32)
    five = rng.uniform(0, 2, size=(5, 3)).astype(np.float32)
    five[:, 2] = 1.0                                              # exactly planar, five distinct positions
    return [("collinear", np.outer(t, np.array([19, 17, 15], np.float32)).astype(np.float32), 3.0),
            ("planar, five positions", five[rng.integers(0, 5, 1000)], 4.0),
            ("identical", np.tile(np.float32([6.6, 6.0, 5.3]), (1000, 1)), 1.0),
            # a radius at which only the coincident points of a grid weigh: beyond it a filled grid is a volume, which a
            # quadric over two of its axes fits without being asked whether that means anything
            ("grid ties", rng.integers(0, 8, size=(2000, 3)).astype(np.float32), 1.0)]


@pytest.fixture(scope="module")
def degenerate_ratios():
    out = {}
    for name, C, radius in _degenerate():
        for k in (6, 8, 32):
            res = M.project(C, 3, None, k, radius, 2, details=True)
            out[name, k] = res[3], res[4]["ratio"]
    return out


def test_degenerate_clouds_are_refused_the_quadric(degenerate_ratios):
    for key, (order, _) in degenerate_ratios.items():
        assert order.max() <= 1, key


def test_the_pivot_ratios_lie_where_the_threshold_was_taken_from(fits, degenerate_ratios):
    # the largest ratio on the degenerate clouds 1.2e-27 (collinear), the smallest on the noisy sphere
    # 8.4e-4; kMlsPivot = 1e-15 is their geometric middle
    worst = max(np.nanmax(r) for _, r in degenerate_ratios.values() if not np.all(np.isnan(r)))
    best = np.nanmin(fits[2][4]["ratio"])
    print("pivot ratios: degenerate <= %.3g, noisy sphere >= %.3g, geometric middle %.3g" % (worst, best, np.sqrt(worst * best)))
    assert worst <= 1e-24 and best >= 1e-4
    assert 0.1 * M.PIVOT <= np.sqrt(max(worst, 1e-300) * best) <= 10 * M.PIVOT
    for (name, k), (_, r) in degenerate_ratios.items():
        if name != "collinear":
            assert np.all(r[~np.isnan(r)] == 0.0), (name, k)           # coincident positions: an exact zero pivot


def test_a_noisy_circle_gets_thinner_and_its_pca_normals_better():
    rng = np.random.default_rng(3)
    th = rng.uniform(0, 2 * np.pi, 4000)
    r = R0 + rng.normal(scale=SIGMA, size=4000)
    P = np.stack([r * np.cos(th), r * np.sin(th)], 1).astype(np.float32)
    rad = np.stack([np.cos(th), np.sin(th)], 1)
    pos, nrm, cur, order = M.project(P, 2, None, 32, 1.0, 2)
    rms_in = np.sqrt(np.mean(_radial(P) ** 2))
    rms_out = np.sqrt(np.mean(_radial(pos) ** 2))
    before = _angle_rms(R.estimate_normals(P, 2, 8)[0], rad)
    after = _angle_rms(R.estimate_normals(pos, 2, 8)[0], rad)
    print("circle: band rms %.4f -> %.4f; PCA normals (k = 8) off radial by %.1f -> %.1f deg rms; fitted normals %.2f deg; "
          "mean |curvature| %.3f" % (rms_in, rms_out, before, after, _angle_rms(nrm, rad), np.abs(cur).mean()))
    assert np.all(order == 2)
    assert rms_out <= 0.5 * rms_in
    assert after <= 0.5 * before
    assert _angle_rms(nrm, rad) <= after


def test_refusals_non_finite_points_guides_and_max_move():
    rng = np.random.default_rng(4)
    P = rng.uniform(0, 10, size=(600, 3)).astype(np.float32)
    P[5, 1] = np.nan
    P[9, 0] = np.inf
    # a radius below the nearest spacing: every point is alone with itself
    pos, nrm, cur, order = M.project(P, 3, None, 8, 1e-3, 2)
    assert np.all(order == 0) and np.array_equal(pos.view(np.uint32), P.view(np.uint32))
    assert np.all(nrm == 0) and np.all(np.isnan(cur))
    q = P[:50].copy() + np.float32(0.1)
    pos, nrm, cur, order = M.project(P, 3, q, 16, 4.0, 2)
    assert np.all(np.isnan(pos[5])) and np.all(np.isnan(pos[9])) and order[5] == 0 and order[9] == 0
    ok = order > 0
    assert ok.sum() >= 40 and np.all(np.abs(np.linalg.norm(nrm[ok].astype(np.float64), axis=1) - 1) < 1e-6)
    g = -nrm.copy()
    g[::3] = np.nan
    p2, n2, c2, o2 = M.project(P, 3, q, 16, 4.0, 2, guide_normals=g)
    flipped = ok & ~np.isnan(g[:, 0])
    assert np.array_equal(n2[flipped], -nrm[flipped]) and np.array_equal(c2[flipped], -cur[flipped])
    assert np.array_equal(n2[~flipped & ok], nrm[~flipped & ok]) and np.array_equal(p2[ok], pos[ok])
    p3 = M.project(P, 3, q, 16, 4.0, 2, max_move=0.01)[0]
    moved = np.linalg.norm(p3[ok].astype(np.float64) - q[ok], axis=1)
    # (the output's fp32 rounding: half an ulp of a coordinate below 16 is 4.8e-7 an axis, 8.3e-7 in length)
    assert moved.max() <= 0.01 + 1e-6 and(np.linalg.norm(pos[ok].astype(np.float64) - q[ok], axis=1) > 0.02).any()
