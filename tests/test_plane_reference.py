"""The numpy restatement of fi_plane_fit / fi_planes_segment (tests/plane_reference.py) held to answers known by hand, so that
the device, which tests/test_gpu_plane.py holds to the restatement bit for bit, is held to them too.  No GPU."""
import numpy as np
import pytest

import cluster_reference as CR
import plane_reference as PR

# the largest component difference between the refit's normal (six Jacobi sweeps) and numpy.linalg.eigh's vector of the same
# moments seen over the clouds of test_refit_against_eigh is 4.44e-16; both differ from the exact vector only
# in rounding, and the bound is 100 times what was seen
EIGH_BOUND = 100 * 4.44e-16


def grid_plane(z=3.0, side=5):
    x, y = np.meshgrid(np.arange(side, dtype=np.float32), np.arange(side, dtype=np.float32))
    return np.stack([x.ravel(), y.ravel(), np.full(side * side, z, np.float32)], axis=1)


def off_points(seed=1, n=10):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, 4.0, (n, 3)).astype(np.float32)
    p[:, 2] = rng.uniform(5.0, 9.0, n)               # none within reach of z = 3
    return p


@pytest.mark.parametrize("refine", [0, 2])
def test_grid_plane_exactly(refine):
    P = np.concatenate([off_points()[:5], grid_plane(), off_points()[5:]])
    model, inl = PR.fit(P, 0.0, refine=refine)
    assert model["found"] == 1 and model["inliers"] == 25 and model["candidates"] == 35 and model["refits"] == refine
    assert model["normal"].tolist() == [0.0, 0.0, 1.0]
    assert model["offset"] == -3.0 and model["rms"] == 0.0
    assert inl.tolist() == [0] * 5 + [1] * 25 + [0] * 5


def test_a_point_at_the_threshold_is_in():
    side = np.float32([[0, 0], [4, 0], [0, 4], [4, 4]])
    above = np.concatenate([side, np.full((4, 1), 4.0, np.float32)], axis=1)
    below = np.concatenate([side, np.full((4, 1), 2.0, np.float32)], axis=1)
    P = np.concatenate([grid_plane(), above, below])
    # only horizontal planes: n_z n_z >= 1
    model, inl = PR.fit(P, 1.0, refine=0, axis=[0, 0, 1], min_cos=1.0)
    assert model["inliers"] == 33 and model["normal"].tolist() == [0.0, 0.0, 1.0] and model["offset"] == -3.0
    assert inl.all()
    just_below = np.nextafter(np.float32(1.0), np.float32(0.0))
    model, inl = PR.fit(P, just_below, refine=0, axis=[0, 0, 1], min_cos=1.0)
    assert model["inliers"] == 25 and model["offset"] == -3.0
    assert inl.tolist() == [1] * 25 + [0] * 8


def test_nothing_to_find():
    line = np.stack([np.arange(20.0), 2.0 * np.arange(20.0), -np.arange(20.0)], axis=1).astype(np.float32)
    model, inl = PR.fit(line, 0.1, max_trials=300)
    assert model["found"] == 0 and model["trials"] == 300 and model["candidates"] == 20 and not inl.any()
    assert model["inliers"] == 0 and model["offset"] == 0.0 and not model["normal"].any()
    P = grid_plane()
    P[3:, 0] = np.nan
    P[1, 1] = np.inf
    model, inl = PR.fit(P, 0.1)
    assert model["found"] == 0 and model["trials"] == 0 and model["candidates"] == 2 and not inl.any()
    keep = np.zeros(25, np.uint8)
    keep[[4, 9]] = 1
    model, _ = PR.fit(grid_plane(), 0.1, mask=keep)
    assert model["found"] == 0 and model["trials"] == 0 and model["candidates"] == 2
    model, _ = PR.fit(grid_plane()[:, :2][:1], 0.1)
    assert model["found"] == 0 and model["candidates"] == 1
    model, inl = PR.fit(np.zeros((0, 3), np.float32), 0.1)
    assert model["found"] == 0 and len(inl) == 0


def test_equal_counts_go_to_the_lower_hypothesis():
    P = np.concatenate([grid_plane(0.0, 4), grid_plane(5.0, 4)])
    P = P[np.random.default_rng(2).permutation(len(P))]
    P64, cand = P.astype(np.float64), np.arange(len(P))
    n, d, valid = PR.hypotheses(P64, cand, 7, np.arange(1024))
    sc = PR.scores(P64, cand, n, d, valid, 0.0)
    assert sc.max() == 16
    top = np.flatnonzero(sc == 16)
    assert {float(abs(d[h])) for h in top} == {0.0, 5.0}                # the tie is real: both planes reach 16
    model, _ = PR.fit(P, 0.0, refine=0, seed=7)
    assert model["inliers"] == 16 and abs(model["offset"]) == abs(d[top[0]])
    other = next(h for h in top if abs(d[h]) != abs(d[top[0]]))
    assert other > top[0]


def test_the_stop_rule():
    rng = np.random.default_rng(3)
    flat = np.concatenate([rng.uniform(0, 31, (300, 2)), np.full((300, 1), 4.0)], axis=1).astype(np.float32)
    model, _ = PR.fit(flat, 0.01, max_trials=5000)
    assert model["trials"] == 1024 and model["inliers"] == 300          # w = 1: r = 0 after the first batch
    # 30 plane points among 270 uniform ones: w ~ 0.1, (1 - w^3)^T <= 0.001 first at T = 7168 of the batch ends
    mixed = np.concatenate([flat[:30], rng.uniform(0, 31, (270, 3)).astype(np.float32)])
    mixed = mixed[rng.permutation(300)]
    model, _ = PR.fit(mixed, 0.01, max_trials=20000, refine=0)
    b, T = model["inliers"], model["trials"]
    assert T % 1024 == 0 and 1024 < T <= 7168 and b >= 30
    assert PR.confident(b, 300, T, 3, 0.999) and not PR.confident(b, 300, T - 1024, 3, 0.999)
    assert PR.confident(30, 300, 7168, 3, 0.999) and not PR.confident(30, 300, 6144, 3, 0.999)
    model, _ = PR.fit(flat, 0.01, max_trials=3000, confidence=0.0)
    assert model["trials"] == 3000


def test_refit_against_eigh():
    worst = 0.0
    clouds = [PR.plane_cloud(s, n, share, ndim) for s, (n, share, ndim) in
              enumerate([(1000, 0.5, 3), (4099, 0.1, 3), (257, 1.0, 3), (1000, 0.5, 2), (300, 1.0, 2)])]
    clouds.append(PR.planted_cloud()[0])
    for P in clouds:
        _, inl = PR.fit(P, 0.1, refine=0)
        X = P[inl != 0].astype(np.float64)
        assert len(X) >= 30
        n, _d = PR.refit(X)
        _c, A = PR.moments(X)
        vec = np.linalg.eigh(A)[1][:, 0]
        vec = vec if vec @ n > 0 else -vec
        worst = max(worst, float(np.abs(vec - n).max()))
    print("refit against eigh: largest component difference %.3g" % worst)
    assert worst <= EIGH_BOUND


def cube_faces(seed=5, per_face=200):
    """six faces of the cube [0, 8]^3, `per_face` points each with coordinates that are multiples of 1/8: exact in fp32"""
    rng = np.random.default_rng(seed)
    pts, face = [], []
    for axis in range(3):
        for side in (0.0, 8.0):
            p = rng.integers(0, 65, (per_face, 3)) / 8.0
            p[:, axis] = side
            pts.append(p)
            face.append(np.full(per_face, 2 * axis + (side > 0)))
    perm = rng.permutation(6 * per_face)
    return np.concatenate(pts).astype(np.float32)[perm], np.concatenate(face)[perm]


def test_the_six_faces_of_a_cube():
    P, face = cube_faces()
    labels, models = PR.segment(P, 0.01, 8, min_inliers=50, max_trials=8192)
    assert len(models) == 6
    assert (labels >= 0).all()
    seen = set()
    for p, model in enumerate(models):
        nz = np.flatnonzero(model["normal"])
        assert len(nz) == 1 and model["normal"][nz[0]] == 1.0             # an axis exactly
        assert model["offset"] in (0.0, -8.0) and model["rms"] == 0.0
        seen.add((int(nz[0]), model["offset"]))
        assert model["inliers"] == int((labels == p).sum()) >= 200 - 40   # (an edge point may have gone to an earlier face)
    assert len(seen) == 6


def test_a_sphere_on_a_floor():
    P, floor = PR.planted_cloud()
    before = CR.cluster(P, 3, 1.5, 1)[2]
    assert before["clusters"] == 1 and before["core"] == 3500             # the floor joins the sphere: nothing to cut
    labels, models = PR.segment(P, 0.15, 1)
    assert len(models) == 1 and (labels[floor] == 0).all()
    model = models[0]
    assert (model["inliers"], model["refits"], model["trials"]) == (2015, 2, 1024)
    took = (labels == 0) & ~floor
    assert int(took.sum()) == 15
    e = P[took].astype(np.float64) @ model["normal"] + model["offset"]
    assert np.abs(e).max() <= 0.15
    assert PR.fit(P, 0.15, refine=0)[0]["inliers"] == 2016                 # the refit is not conditional on the count
    rest = P[labels < 0]
    after, _, stats = CR.cluster(rest, 3, 1.5, 1)
    assert np.bincount(after[after >= 0]).max() == 1485 == len(rest)       # the rest of the sphere, one cluster


def test_arguments():
    P = grid_plane()
    for bad in (dict(threshold=-1.0), dict(threshold=np.nan), dict(threshold=np.inf), dict(max_trials=0),
                dict(max_trials=2 ** 20 + 1), dict(confidence=1.0), dict(confidence=-0.1), dict(refine=-1), dict(refine=17),
                dict(min_cos=1.5), dict(min_cos=-0.5), dict(min_cos=0.5, axis=[0, 0, 0]), dict(min_cos=0.5, axis=[np.nan, 0, 1])):
        args = dict(threshold=0.1)
        args.update(bad)
        with pytest.raises(PR.Invalid):
            PR.fit(P, **args)
    with pytest.raises(PR.Invalid):
        PR.fit(P[:, :1], 0.1)
    with pytest.raises(PR.Invalid):
        PR.segment(P, 0.1, 0)
    with pytest.raises(PR.Invalid):
        PR.segment(P, 0.1, 1, min_inliers=-1)
