"""The numpy restatement of fi_shape_fit / fi_shapes_segment (tests/shape_reference.py) held to answers known by hand and to
the two planted scenes of DESIGN.md 4.26, so that the device, which tests/test_gpu_shape.py holds to the restatement bit for
bit, is held to them too.  No GPU."""
import numpy as np
import pytest

import shape_reference as SR


def six_points(r=2.0, shift=(3.0, -1.0, 5.0)):
    """(+-r, 0, 0), (0, +-r, 0), (0, 0, +-r) about `shift`: exact in fp32"""
    p = np.concatenate([r * np.eye(3), -r * np.eye(3)])
    return (p + np.asarray(shift)).astype(np.float32)


def far_points(seed=1, n=8):
    return np.random.default_rng(seed).uniform(20.0, 30.0, (n, 3)).astype(np.float32)      # none within reach


def ring_cylinder(levels=5):
    """(+-1, 0, z), (0, +-1, z), z = 0 .. levels - 1, with their radial normals: a cylinder of radius 1 about the z axis"""
    ring = np.float32([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]])
    P = np.concatenate([ring + np.float32([0, 0, z]) for z in range(levels)])
    return P, np.tile(ring, (levels, 1))


@pytest.mark.parametrize("refine", [0, 2])
def test_six_points_give_the_centre_and_radius_exactly(refine):
    P = np.concatenate([far_points()[:4], six_points(), far_points()[4:]])
    model, inl = SR.fit(P, SR.SPHERE, 0.0, refine=refine, r_max=3.0)
    assert model["found"] == 1 and model["kind"] == SR.SPHERE and model["inliers"] == 6 and model["candidates"] == 14
    assert model["refits"] == refine
    assert model["center"].tolist() == [3.0, -1.0, 5.0] and model["radius"] == 2.0 and model["rms"] == 0.0
    assert not model["axis"].any() and not model["extent"].any()
    assert inl.tolist() == [0] * 4 + [1] * 6 + [0] * 4
    # the circle in the plane of the first four, as a 2-D cloud
    C = six_points()[[0, 1, 3, 4]][:, :2]
    model, inl = SR.fit(C, SR.SPHERE, 0.0, refine=refine)
    assert model["center"].tolist() == [3.0, -1.0, 0.0] and model["radius"] == 2.0 and model["inliers"] == 4 and inl.all()


def test_coplanar_points_and_parallel_normals_make_no_hypothesis():
    flat = six_points()[[1, 2, 4, 5]]                                   # x = 3: four points of one plane
    c, a, r, valid = SR.hypotheses(SR.SPHERE, flat.astype(np.float64), None, np.arange(4), 0, np.arange(200))
    assert not valid.any()
    model, inl = SR.fit(flat, SR.SPHERE, 0.1, max_trials=300)
    assert (model["found"], model["trials"], model["candidates"]) == (0, 300, 4) and not inl.any()
    assert model["radius"] == 0.0 and not model["center"].any()
    x, ok = SR.cramer(np.array([[[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 1.0, 5.0]]]), np.ones((1, 3)))
    assert not ok[0]
    x, ok = SR.cramer(np.array([[[2.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 8.0]]]), np.array([[2.0, 2.0, 2.0]]))
    assert ok[0] and x[0].tolist() == [1.0, 0.5, 0.25]
    x, ok = SR.cramer(np.array([[[2.0, 1.0], [1.0, 1.0]]]), np.array([[3.0, 2.0]]))
    assert ok[0] and x[0].tolist() == [1.0, 1.0]
    P, N = ring_cylinder()
    same = np.tile(np.float32([[0, 3, 0]]), (len(P), 1))                # every normal along y
    model, _ = SR.fit(P, SR.CYLINDER, 0.1, normals=same, max_trials=300)
    assert (model["found"], model["trials"], model["candidates"]) == (0, 300, 20)
    opposite = same * np.where(np.arange(len(P)) % 2, -1, 1)[:, None].astype(np.float32)
    assert SR.fit(P, SR.CYLINDER, 0.1, normals=opposite, max_trials=300)[0]["found"] == 0


def test_the_radius_limits():
    P = np.concatenate([six_points(), far_points()])
    assert SR.fit(P, SR.SPHERE, 0.0, r_min=2.0, r_max=2.0)[0]["inliers"] == 6           # both ends are in
    for lim in (dict(r_min=2.5, r_max=3.0), dict(r_max=1.5)):
        model, _ = SR.fit(P, SR.SPHERE, 0.0, **lim)
        assert model["inliers"] < 6 and (not model["found"] or lim.get("r_min", 0.0) <= model["radius"] <= lim["r_max"])
    model, _ = SR.fit(six_points(), SR.SPHERE, 0.0, r_min=2.5)
    assert model["found"] == 0 and model["trials"] == 1024
    Pc, Nc = ring_cylinder()
    assert SR.fit(Pc, SR.CYLINDER, 0.0, normals=Nc, r_min=1.0, r_max=1.0)[0]["inliers"] == 20
    assert SR.fit(Pc, SR.CYLINDER, 0.0, normals=Nc, r_min=1.5)[0]["found"] == 0


def test_the_band_and_its_edges():
    lo2, hi2 = SR.band(np.array([2.0]), 3.0)
    assert lo2[0] == 0.0 and hi2[0] == 25.0                                              # lo is held at 0
    lo2, hi2 = SR.band(np.array([2.0]), 1.0)
    assert lo2[0] == 1.0 and hi2[0] == 9.0
    X = np.float64([[3, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, -2]])
    c, a, r = np.zeros((1, 3)), np.zeros((1, 3)), np.array([2.0])
    assert SR.inside(SR.SPHERE, X, None, c, a, r, 1.0, 0.0)[0][0].tolist() == [True, True, False, True]     # a point on either edge is in
    just_below = np.nextafter(np.float32(1.0), np.float32(0.0))
    assert SR.inside(SR.SPHERE, X, None, c, a, r, just_below, 0.0)[0][0].tolist() == [False, False, False, True]
    assert SR.inside(SR.SPHERE, X, None, c, a, r, 3.0, 0.0)[0][0].tolist() == [True, True, True, True]      # the centre itself: s = 0 = lo2
    # a cylinder about z: the same distances across the axis, wherever along it
    X = np.float64([[3, 0, 7], [0, 1, -4], [0, 0, 9], [0, -2, 1]])
    a = np.array([[0.0, 0.0, 1.0]])
    assert SR.inside(SR.CYLINDER, X, None, c, a, r, 1.0, 0.0)[0][0].tolist() == [True, True, False, True]
    assert SR.inside(SR.CYLINDER, X, None, c, a, r, just_below, 0.0)[0][0].tolist() == [False, False, False, True]
    # the angle test: (u . g)^2 >= mc^2 (g . g), either way round, false on the axis itself
    U = np.float64([[-1, 0, 0], [1, 0, 0], [0, 0, 1], [0.6, -0.8, 0]])
    mc = np.float32(0.8)
    got = SR.inside(SR.CYLINDER, X, U, c, a, r, 3.0, mc)[0][0].tolist()
    assert got == [True, False, False, bool(0.8 * 0.8 * 4.0 >= np.float64(mc) ** 2 * 4.0)]


def test_the_stop_rule():
    # w = 1 / 2.  S = 4: 0.9375^T <= 0.001 first at T = 108; S = 2: 0.75^T first at T = 25
    assert SR.confident(50, 100, 108, 4, 0.999) and not SR.confident(50, 100, 107, 4, 0.999)
    assert SR.confident(50, 100, 25, 2, 0.999) and not SR.confident(50, 100, 24, 2, 0.999)
    assert SR.confident(50, 100, 52, 3, 0.999) and not SR.confident(50, 100, 51, 3, 0.999)
    assert SR.sample_size(SR.SPHERE, 3) == 4 and SR.sample_size(SR.SPHERE, 2) == 3 and SR.sample_size(SR.CYLINDER, 3) == 2
    for kind, D, share in ((SR.SPHERE, 3, 0.26), (SR.CYLINDER, 3, 0.08)):
        S = SR.sample_size(kind, D)
        P, N = SR.shape_cloud(77, 1000, share, kind, D)
        model, _ = SR.fit(P, kind, 0.05, normals=N, max_trials=20000, refine=0, seed=5)
        b, T = model["inliers"], model["trials"]
        assert T == 2048 and SR.confident(b, 1000, T, S, 0.999) and not SR.confident(b, 1000, T - 1024, S, 0.999)
        model, _ = SR.fit(P, kind, 0.05, normals=N, max_trials=3000, confidence=0.0)
        assert model["trials"] == 3000
    P, N = SR.shape_cloud(3, 300, 1.0, SR.SPHERE, 3)
    assert SR.fit(P, SR.SPHERE, 0.05, max_trials=5000)[0]["trials"] == 1024               # w = 1: r = 0 after the first batch


def test_the_axis_sign_and_the_extent():
    P, N = ring_cylinder()
    signs = set()
    for seed in range(6):
        c, a, r, valid = SR.hypotheses(SR.CYLINDER, P.astype(np.float64), N.astype(np.float64), np.arange(20), seed, np.arange(64))
        signs |= {float(z) for z in a[valid][:, 2]}
        model, inl = SR.fit(P, SR.CYLINDER, 0.0, normals=N, refine=0, seed=seed)
        assert model["found"] == 1 and model["inliers"] == 20 and inl.all() and model["radius"] == 1.0 and model["rms"] == 0.0
        assert model["axis"].tolist() == [0.0, 0.0, 1.0]                   # whichever way round the two normals were drawn
        assert model["center"][:2].tolist() == [0.0, 0.0]
        assert model["extent"].tolist() == [0.0 - model["center"][2], 4.0 - model["center"][2]]
    assert signs == {1.0, -1.0}
    model, _ = SR.fit(P, SR.CYLINDER, 0.0, normals=N, refine=2)
    assert model["refits"] == 2 and model["axis"].tolist() == [0.0, 0.0, 1.0] and model["center"].tolist() == [0.0, 0.0, 2.0]
    assert model["radius"] == 1.0 and model["extent"].tolist() == [-2.0, 2.0]
    # the same cylinder laid along -x: the largest component is made positive, the extent follows
    Q, M = P[:, [2, 0, 1]] * np.float32([-1, 1, 1]), N[:, [2, 0, 1]]
    model, _ = SR.fit(Q, SR.CYLINDER, 0.0, normals=M, refine=0, seed=1)
    assert model["axis"].tolist() == [1.0, 0.0, 0.0] and model["extent"].tolist() == [-4.0 - model["center"][0], 0.0 - model["center"][0]]


def test_unusable_normals_are_no_candidates():
    P, N = ring_cylinder()
    N = N.copy()
    N[3] = 0.0
    N[7, 1] = np.nan
    N[9, 2] = np.inf
    for kind in (SR.SPHERE, SR.CYLINDER):
        model, inl = SR.fit(P, kind, 0.0, normals=N)
        assert model["candidates"] == 17 and not inl[[3, 7, 9]].any()
    assert SR.fit(P, SR.SPHERE, 0.0)[0]["candidates"] == 20
    U, ok = SR.unit_normals(np.float32([[3, 0, 4], [0, 0, 0]]))
    assert U[0].tolist() == [0.6, 0.0, 0.8] and ok.tolist() == [True, False]


def _axis_angle(a, b):
    return float(np.degrees(np.arccos(min(1.0, abs(float(a @ b))))))


def test_the_planted_sphere():
    """scene (a) of DESIGN.md 4.26.  The conditions are caps set before anything ran; the figures are printed"""
    P, N, planted = SR.planted_sphere()
    first, _ = SR.fit(P, SR.SPHERE, 0.05, r_min=0.5, r_max=5.0, refine=0)
    model, inl = SR.fit(P, SR.SPHERE, 0.05, r_min=0.5, r_max=5.0)
    inl = inl.astype(bool)
    off, dr = float(np.linalg.norm(model["center"] - [1.0, 2.0, 2.0])), abs(model["radius"] - 2.0)
    print("scene (a): best hypothesis centre %.4f off, %d inliers; after %d refits centre %.2e off, radius %.2e off, %d of %d planted in, "
          "%d foreign" % (np.linalg.norm(first["center"] - [1.0, 2.0, 2.0]), first["inliers"], model["refits"], off, dr,
                          inl[planted].sum(), planted.sum(), inl[~planted].sum()))
    assert model["found"] == 1 and model["trials"] == 1024
    assert off <= 0.05 and dr <= 0.05
    assert inl[planted].sum() >= 0.95 * planted.sum()
    assert inl[~planted].sum() <= 0.05 * inl.sum()


def test_the_planted_cylinder():
    """scene (b) of DESIGN.md 4.26"""
    P, N, planted = SR.planted_cylinder()
    first, _ = SR.fit(P, SR.CYLINDER, 0.05, r_min=0.1, r_max=2.0, normals=N, refine=0)
    model, inl = SR.fit(P, SR.CYLINDER, 0.05, r_min=0.1, r_max=2.0, normals=N)
    inl = inl.astype(bool)
    angle = _axis_angle(model["axis"], SR.CYL_AXIS)
    apart = float(np.linalg.norm(np.cross(SR.CYL_POINT - model["center"], model["axis"])) / np.linalg.norm(model["axis"]))
    dr = abs(model["radius"] - 0.5)
    print("scene (b): best hypothesis %d inliers, axis %.2f degrees off; after %d refits axis %.3f degrees off, %.2e from the planted axis "
          "point, radius %.2e off, %d of %d planted in, %d foreign" % (first["inliers"], _axis_angle(first["axis"], SR.CYL_AXIS),
                                                                       model["refits"], angle, apart, dr, inl[planted].sum(), planted.sum(),
                                                                       inl[~planted].sum()))
    assert model["found"] == 1
    assert angle <= 2.0 and apart <= 0.05 and dr <= 0.05
    assert inl[planted].sum() >= 0.95 * planted.sum()
    assert inl[~planted].sum() <= 0.05 * inl.sum()


def test_two_spheres_peeled_off():
    rng = np.random.default_rng(8)
    a, _ = SR.sphere_part(rng, 700, [2.5, 2.5, 2.5], 2.0, 0.02)
    b, _ = SR.sphere_part(rng, 300, [7.0, 6.0, 7.0], 1.0, 0.02)
    P = np.concatenate([a, b, rng.uniform(0.0, 9.0, (200, 3))]).astype(np.float32)
    labels, models = SR.segment(P, SR.SPHERE, 0.05, 3, min_inliers=250)
    assert len(models) == 2 and (labels[:700] == 0).all() and (labels[700:1000] == 1).all()
    assert abs(models[0]["radius"] - 2.0) < 0.01 and abs(models[1]["radius"] - 1.0) < 0.01
    labels, models = SR.segment(P, SR.SPHERE, 0.05, 3, min_inliers=500)
    assert len(models) == 1 and set(labels.tolist()) == {-1, 0}
    first, inl = SR.fit(P, SR.SPHERE, 0.05)
    assert first["inliers"] == models[0]["inliers"] and np.array_equal(inl != 0, labels == 0)


def test_arguments():
    P, N = ring_cylinder()
    for bad in (dict(threshold=-1.0), dict(threshold=np.nan), dict(threshold=np.inf), dict(max_trials=0), dict(max_trials=2 ** 20 + 1),
                dict(confidence=1.0), dict(confidence=-0.1), dict(refine=-1), dict(refine=17), dict(r_min=-0.5), dict(r_min=2.0, r_max=1.0),
                dict(r_min=np.nan), dict(r_max=np.nan), dict(normal_cos=1.5), dict(normal_cos=-0.5), dict(normal_cos=np.nan)):
        args = dict(threshold=0.1, normals=N)
        args.update(bad)
        for kind in (SR.SPHERE, SR.CYLINDER):
            with pytest.raises(SR.Invalid):
                SR.fit(P, kind, **args)
    with pytest.raises(SR.Invalid):
        SR.fit(P, 2, 0.1)
    with pytest.raises(SR.Invalid):
        SR.fit(P, SR.CYLINDER, 0.1)                                     # a cylinder without normals
    with pytest.raises(SR.Invalid):
        SR.fit(P, SR.SPHERE, 0.1, normal_cos=0.5)                       # an angle without normals
    with pytest.raises(SR.Unsupported):
        SR.fit(P[:, :2], SR.CYLINDER, 0.1, normals=N[:, :2])
    with pytest.raises(SR.Invalid):
        SR.fit(P[:, :1], SR.SPHERE, 0.1)
    with pytest.raises(SR.Invalid):
        SR.segment(P, SR.SPHERE, 0.1, 0)
    with pytest.raises(SR.Invalid):
        SR.segment(P, SR.SPHERE, 0.1, 1, min_inliers=-1)
    assert SR.fit(P, SR.SPHERE, 0.1, r_max=np.inf)[0]["found"] == 1
    model, inl = SR.fit(np.zeros((0, 3), np.float32), SR.SPHERE, 0.1)
    assert model["found"] == 0 and len(inl) == 0
