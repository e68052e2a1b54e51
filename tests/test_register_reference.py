"""The numpy restatement of the registration contract (tests/register_reference.py; include/fi_hip.h fi_mesh_register,
DESIGN.md 4.18) held to facts known without it: recovered transforms, the unknowns a flat target cannot see, what a robust
loss buys, the counts, the Cholesky against numpy.linalg.solve and the Cayley map against Rodrigues' formula.  No GPU.  The
figures measured with the restatement stand beside each bound (and in DESIGN.md 4.18)."""
import functools

import numpy as np

import register_reference as G


@functools.lru_cache(maxsize=None)
def cube():
    return G.cube_case()


def _off(result, truth):
    R, t = truth
    D = len(t)
    return np.abs(result["transform"][:D, :D] - R).max(), np.abs(result["transform"][:D, D] - t).max()


def _orthogonal(result):
    D = result["transform"].shape[0] - 1
    R = result["transform"][:D, :D]
    return np.abs(R @ R.T - np.eye(D)).max()


def test_cube_plane_recovers_the_transform():
    """measured: 5 iterations, R off by 2.0e-9, t by 3.3e-8, R R^T - I 6.7e-16, rms 1.0e-7 (one fp32 ulp at 11.25 is 9.5e-7);
    a 25 degree start 7 iterations, a 40 degree start 8"""
    v, t, _pts, _nrm, src, truth = cube()
    r = G.register(G.Target(v, t), src)
    assert r["converged"] == 1 and r["iterations"] <= 8 and r["fixed_mask"] == 0
    dr, dt = _off(r, truth)
    assert dr < 1e-6 and dt < 1e-5, (dr, dt)
    assert _orthogonal(r) < 1e-14
    assert r["rms"] < 1e-5 and r["rms"] == r["weighted_rms"]
    assert r["counted"] == r["queries"] == 600 and r["beyond"] == r["invalid"] == r["degenerate"] == 0
    assert r["transformed"].dtype == np.float32 and r["transformed"].shape == (600, 3) and r["distances"].max() < 1e-5
    v, t, _pts, _nrm, far, truth = G.cube_case(degrees=40.0)
    r = G.register(G.Target(v, t), far)
    dr, dt = _off(r, truth)
    assert r["converged"] == 1 and r["iterations"] <= 10 and dr < 1e-6 and dt < 1e-5


def test_cube_point_mode_creeps_where_plane_mode_lands():
    """measured: the rms before each of 10 point-to-point steps falls from 0.317 to 0.0372, 0.0302 behind them; plane mode
    ends at 1.0e-7"""
    v, t, _pts, _nrm, src, _truth = cube()
    before = []
    r = G.register(G.Target(v, t), src, mode=G.POINT, max_iterations=10, history=before)
    rms = [x[0] for x in before] + [r["rms"]]
    assert r["iterations"] == 10 and r["converged"] == 0
    assert all(a > b for a, b in zip(rms, rms[1:])), rms
    assert r["rms"] > G.register(G.Target(v, t), src)["rms"]


def test_flat_grid_fixes_the_unknowns_it_cannot_see():
    """measured: 3 iterations; fixed_mask 0b011100 (omega_2, tau_0, tau_1) at every step"""
    v, t, src = G.flat_case()
    r = G.register(G.Target(v, t), src)
    assert r["converged"] == 1 and r["iterations"] <= 4 and r["fixed_mask"] == 0b011100
    T = r["transform"]
    # no turn about z and no slide along x or y: the image of the pivot keeps its x and y, the x axis stays the x axis
    g0, _any = G.pivot(src)
    assert np.abs((T[:3, :3] @ g0 + T[:3, 3])[:2] - g0[:2]).max() < 1e-9
    assert abs(T[1, 0]) < 1e-9 and abs(T[0, 1]) < 1e-9 and abs(T[0, 0] - 1.0) < 1e-9
    assert r["rms"] < 1e-6 and np.abs(r["transformed"][:, 2] - 3.0).max() < 1e-5


def test_rectangle_2d():
    """measured: 4 iterations, R off by 6.8e-10, t by 1.9e-8, rms 1.1e-7"""
    v, s, _on, _nrm, src, truth = G.rectangle_case()
    r = G.register(G.Target(v, s), src)
    assert r["transform"].shape == (3, 3) and np.array_equal(r["transform"][2], (0.0, 0.0, 1.0))
    assert r["converged"] == 1 and r["iterations"] <= 8 and r["fixed_mask"] == 0
    dr, dt = _off(r, truth)
    assert dr < 1e-6 and dt < 1e-5, (dr, dt)
    assert _orthogonal(r) < 1e-14 and r["rms"] < 1e-5


def test_point_set_targets():
    """measured: the cube's own sample points with their face normals as the target, plane mode: 4 iterations, R off by
    6.2e-9"""
    _v, _t, pts, nrm, src, truth = cube()
    r = G.register(G.Target(points=pts, normals=nrm), src)
    dr, dt = _off(r, truth)
    assert r["converged"] == 1 and dr < 1e-6 and dt < 1e-5
    r = G.register(G.Target(points=pts), src, mode=G.POINT, max_iterations=3)
    assert r["counted"] == 600 and r["iterations"] == 3
    try:
        G.register(G.Target(points=pts), src)
        assert False, "plane mode without normals"
    except G.Invalid:
        pass


def test_outliers_and_tukey():
    """measured: plain least squares R off by 8.5e-3, t by 8.1e-2; Tukey at scale 0.1 R off by 1.5e-9, t by 2.2e-8"""
    v, t, src, truth = G.outlier_case()
    plain = G.register(G.Target(v, t), src, max_distance=1.5)
    assert _off(plain, truth)[0] > 1e-3
    robust = G.register(G.Target(v, t), src, max_distance=1.5, loss=G.TUKEY, scale=0.1)
    dr, dt = _off(robust, truth)
    assert dr < 1e-6 and dt < 1e-5, (dr, dt)
    assert robust["weighted_rms"] < 1e-5 < robust["rms"]


def test_counts():
    v, t, _pts, _nrm, src, _truth = cube()
    src = src.copy()
    src[7, 1], src[9] = np.nan, np.inf
    flat = np.array([[20, 20, 20], [21, 20, 20], [22, 20, 20]], np.float32)
    v2 = np.concatenate([v, flat])
    t2 = np.concatenate([t, [[len(v), len(v) + 1, len(v) + 2]]])
    src = np.concatenate([src, [[20.5, 20.1, 20.0]]]).astype(np.float32)
    for mode, degenerate in ((G.PLANE, 1), (G.POINT, 0)):
        r = G.register(G.Target(v2, t2), src, mode=mode, max_iterations=0, max_distance=0.8)
        assert r["counted"] + r["beyond"] + r["invalid"] + r["degenerate"] == r["queries"] == 601
        assert r["invalid"] == 2 and r["degenerate"] == degenerate and r["beyond"] > 0
        assert np.isnan(r["distances"][[7, 9]]).all() and r["iterations"] == 0
    start = np.eye(4)
    start[:3, 3] = (100.0, 0.0, 0.0)
    r = G.register(G.Target(v, t), src, max_distance=1.0, initial=start)       # nothing within reach: the transform stays
    assert r["counted"] == 0 and r["iterations"] == 0 and np.array_equal(r["transform"], start) and r["rms"] == 0.0
    r = G.register(G.Target(v, t), np.full((5, 3), np.nan, np.float32))
    assert r["invalid"] == 5 and r["iterations"] == 0 and np.array_equal(r["transform"], np.eye(4))
    for bad in (dict(max_iterations=-1), dict(max_distance=-1.0), dict(max_distance=np.nan), dict(rotation_tolerance=np.nan),
                dict(translation_tolerance=-1e-3), dict(mode=2), dict(loss=3), dict(loss=G.HUBER), dict(loss=G.HUBER, scale=-1.0),
                dict(initial=np.full((4, 4), np.inf))):
        try:
            G.register(G.Target(v, t), src, **bad)
            assert False, bad
        except G.Invalid:
            pass


def test_cholesky_against_numpy():
    rng = np.random.default_rng(3)
    for U in (3, 6):
        A = rng.normal(size=(40, U))
        M, b = A.T @ A, rng.normal(size=U)
        delta, mask = G.solve(np.triu(M), b)
        want = np.linalg.solve(M, -b)
        assert mask == 0 and np.abs(delta - want).max() <= 1e-10 * np.abs(want).max()
        # an unknown nothing depends on is fixed at 0 and the others are solved without it
        M0 = M.copy()
        M0[2, :], M0[:, 2] = 0.0, 0.0
        delta, mask = G.solve(np.triu(M0), b)
        keep = [k for k in range(U) if k != 2]
        want = np.linalg.solve(M[np.ix_(keep, keep)], -b[keep])
        assert mask == 0b100 and delta[2] == 0.0 and np.abs(delta[keep] - want).max() <= 1e-10 * np.abs(want).max()
    assert G.solve(np.zeros((6, 6)), np.zeros(6))[1] == 0b111111


def test_cayley_against_rodrigues():
    rng = np.random.default_rng(4)
    for scale in (1e-1, 1e-2, 1e-3):
        w = rng.normal(size=3) * scale
        angle = np.linalg.norm(w)
        R = G.cayley(3, w)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1.0) < 1e-15   # a rotation for any step
        # the same axis, the angle 2 atan(|w| / 2) = |w| - |w|^3 / 12 + ...: equal to second order
        assert np.abs(R - G.rotation(w, np.rad2deg(angle))).max() < angle ** 3 / 6
        assert np.abs(R - G.rotation(w, np.rad2deg(2 * np.arctan(angle / 2)))).max() < 1e-15
        c, s = np.cos(w[0]), np.sin(w[0])
        assert np.abs(G.cayley(2, w[:1]) - np.array([[c, -s], [s, c]])).max() < abs(w[0]) ** 3 / 6
