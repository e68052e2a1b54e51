"""Sphere, circle and cylinder segmentation on the device (fi_shape.hip through segment_sphere, segment_cylinder,
segment_shapes and the raw fi_shape_fit / fi_shapes_segment) against the numpy restatement of the contract
(tests/shape_reference.py): inlier masks and labels array-equal, every integer of a model equal and every double as a bit
pattern.  The sizes where a tile of the score, a chunk of the tree sums and a wave end, a cloud past the score grid's cap,
trial counts on both sides of a batch, the stop rule after the second batch, inlier shares of a tenth, a half and all, refits
(one that loses inliers, one the radius limit ends), a mask, non-finite points and unusable normals, duplicates, the radius
limits, the angle test, several shapes peeled off, the planted scenes, repeated calls, the error codes, and device tensors
through a child process."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import shape_reference as SR

pytestmark = pytest.mark.gpu

MODELS = [("sphere", 3), ("sphere", 2), ("cylinder", 3)]
COUNTS = [63, 64, 65, 255, 256, 257, 1000, 4099]            # both sides of a wave (64), of a tile and a chunk (256); 17 chunks
MANY = [16384, 16385]                                       # all inliers: 64 chunks, one load of the ordered sum, and a 65th
TRIALS = [1, 1023, 1024, 1025, 3000]                        # both sides of a batch (1024), two batches and a partial one
SHARES = [0.1, 0.5, 1.0]
INTS = ("found", "refits", "inliers", "candidates", "trials")
KIND = {"sphere": SR.SPHERE, "cylinder": SR.CYLINDER}
COS20 = float(np.float32(math.cos(math.radians(20.0))))


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _bits(x):
    return np.asarray(x, np.float64).reshape(-1).view(np.uint64).tolist()


def _doubles(model, D):
    """every double of a model in one list: the restatement's dict, the Python API's or a raw row"""
    out = list(np.asarray(model["center"], np.float64)[:D]) + [model["radius"], model["rms"]]
    if "axis" in model:
        out += list(model["axis"]) + list(model["extent"])
    return out


def _same_model(got, want, D, kind, what=""):
    for key in INTS:
        assert int(got[key]) == int(want[key]), (what, key, got, want)
    assert got["center"].dtype == np.float64 and got["center"].shape == (D,), what
    if kind != "cylinder":
        want = {k: v for k, v in want.items() if k not in ("axis", "extent")}
        assert "axis" not in got or not np.any(got["axis"]), what
        got = {k: v for k, v in got.items() if k not in ("axis", "extent")}
    assert _bits(_doubles(got, D)) == _bits(_doubles(want, D)), (what, got, want)


def _cos(max_angle):
    return 0.0 if max_angle is None else float(np.float32(math.cos(math.radians(max_angle))))


def _row(m, D):
    """a raw fi_shape_model as the restatement's dict"""
    return {"found": m.found, "kind": m.kind, "refits": m.refits, "inliers": m.inliers, "candidates": m.candidates, "trials": m.trials,
            "center": np.array(m.center[:D], np.float64), "rest_of_center": list(m.center[D:]), "axis": np.array(m.axis[:], np.float64),
            "radius": m.radius, "extent": np.array(m.extent[:], np.float64), "rms": m.rms}


def _raw(kind, P, N, mask, max_shapes=None, min_inliers=0, threshold=0.05, r_min=0.0, r_max=math.inf, max_angle=None, max_trials=1024,
         confidence=0.999, refine=2, seed=0, ndim=None, memory=0, code_of_kind=None):
    """the C entries with host buffers -> (code, model dict or list of them, inliers or labels)"""
    from field_interpolation_amd import _capi
    L = _capi.lib()
    P = np.ascontiguousarray(P, np.float32)
    n, D = P.shape[0], (P.shape[1] if ndim is None else ndim)
    opt = _capi.FiShapeOptions(KIND[kind] if code_of_kind is None else code_of_kind, threshold, r_min, r_max, _cos(max_angle), max_trials,
                               confidence, refine, seed)
    nr = None if N is None else np.ascontiguousarray(N, np.float32)
    mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    if max_shapes is None:
        model, inl = _capi.FiShapeModel(), np.full(n, 7, np.uint8)
        code = L.fi_shape_fit(D, n, ptr(P), ptr(nr), ptr(mk), C.byref(opt), C.byref(model), ptr(inl), memory)
        return code, _row(model, P.shape[1]), inl
    rows, labels, found = (_capi.FiShapeModel * max(max_shapes, 1))(), np.full(n, 7, np.int32), C.c_int(-1)
    code = L.fi_shapes_segment(D, n, ptr(P), ptr(nr), ptr(mk), C.byref(opt), max_shapes, min_inliers, ptr(labels), rows, C.byref(found), memory)
    return code, [_row(rows[i], P.shape[1]) for i in range(max(found.value, 0))], labels


def _same_row(row, want, D, what):
    """a raw row holds every field of the restatement's model, the unused ones 0"""
    assert row["kind"] == want["kind"] and row["rest_of_center"] == [0.0] * (3 - D), (what, row)
    _same_model(row, want, D, "cylinder", what)               # (all the doubles: a sphere's axis and extent are zeros in both)


def _check_fit(fi, kind, P, N, what="", mask=None, max_angle=None, **kw):
    """segment_sphere / segment_cylinder and the raw entry against the restatement"""
    D = P.shape[1]
    want, want_inl = SR.fit(P, KIND[kind], normals=N, mask=mask, normal_cos=_cos(max_angle), **kw)
    if kind == "cylinder":
        model, inl = fi.segment_cylinder(P, N, mask=mask, max_angle=max_angle, **kw)
    else:
        model, inl = fi.segment_sphere(P, normals=N, mask=mask, max_angle=max_angle, **kw)
    assert inl.dtype == np.bool_ and np.array_equal(inl, want_inl.astype(bool)), (what, np.flatnonzero(inl != want_inl.astype(bool))[:5])
    assert model["kind"] == kind and ("axis" in model) == (kind == "cylinder")
    _same_model(model, want, D, kind, what)
    code, row, inl = _raw(kind, P, N, mask, max_angle=max_angle, **kw)
    assert code == 0 and np.array_equal(inl, want_inl), what
    _same_row(row, want, D, what)
    return want, want_inl


def _check_segment(fi, kind, P, N, max_shapes, what="", mask=None, max_angle=None, **kw):
    D = P.shape[1]
    want_labels, want = SR.segment(P, KIND[kind], max_shapes=max_shapes, normals=N, mask=mask, normal_cos=_cos(max_angle), **kw)
    labels, models = fi.segment_shapes(P, kind, max_shapes=max_shapes, normals=N, mask=mask, max_angle=max_angle, **kw)
    assert labels.dtype == np.int32 and np.array_equal(labels, want_labels), what
    code, rows, raw_labels = _raw(kind, P, N, mask, max_shapes=max_shapes, max_angle=max_angle, **kw)
    assert code == 0 and np.array_equal(raw_labels, want_labels), what
    assert len(models) == len(rows) == len(want), (what, len(models), len(rows), len(want))
    for g, r, w in zip(models, rows, want):
        _same_model(g, w, D, kind, what)
        _same_row(r, w, D, what)
    return want_labels, want


def _cloud(kind, D, seed, n, share):
    """positions and, for a cylinder, normals"""
    P, N = SR.shape_cloud(seed, n, share, KIND[kind], D)
    return P, (N if kind == "cylinder" else None)


@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("kind,D", MODELS)
def test_sizes(fi, kind, D, share):
    S = SR.sample_size(KIND[kind], D)
    for n in [S - 1, S] + COUNTS + (MANY if share == 1.0 else []):
        P, N = _cloud(kind, D, 100 * D + n, n, share)
        want, _ = _check_fit(fi, kind, P, N, (kind, D, n, share), threshold=0.05, max_trials=1025, refine=1, seed=n)
        assert want["found"] == (1 if n >= S else 0) and want["candidates"] == n
        if n == S - 1:
            assert want["trials"] == 0
        if n in MANY:
            assert want["inliers"] == n


@pytest.mark.parametrize("kind,D", MODELS)
def test_a_cloud_past_the_cap_of_the_score_grid(fi, kind, D):
    n = 131072 + 257                                          # 512 tiles of 256 and two more: a workgroup walks a second tile
    P, N = _cloud(kind, D, 9 + D, n, 0.5)
    want, _ = _check_fit(fi, kind, P, N, (kind, D, "cap"), threshold=0.05, max_trials=64, refine=1)
    assert want["found"] == 1 and want["candidates"] == n


@pytest.mark.parametrize("confidence", [0.0, 0.999])
@pytest.mark.parametrize("kind,D", MODELS)
def test_trial_counts(fi, kind, D, confidence):
    P, N = _cloud(kind, D, 7 + D, 1000, 0.5)
    for trials in TRIALS:
        want, _ = _check_fit(fi, kind, P, N, (kind, D, trials), threshold=0.05, max_trials=trials, confidence=confidence, seed=3)
        assert want["trials"] == (trials if confidence == 0.0 else min(trials, 1024))


@pytest.mark.parametrize("kind,D,share", [("sphere", 3, 0.26), ("sphere", 2, 0.17), ("cylinder", 3, 0.08)])
def test_the_stop_rule_ends_after_the_second_batch(fi, kind, D, share):
    """an inlier share w with (1 - w^S)^1024 above 0.001 and (1 - w^S)^2048 below it"""
    P, N = _cloud(kind, D, 77, 1000, share)
    want, _ = _check_fit(fi, kind, P, N, (kind, D, "stop"), threshold=0.05, max_trials=20000, refine=0, seed=5)
    assert want["trials"] == 2048


@pytest.mark.parametrize("kind,D", MODELS)
def test_refits_and_a_mask(fi, kind, D):
    P, N = _cloud(kind, D, 20 + D, 1000, 0.5)
    for refine in (0, 1, 3):
        want, _ = _check_fit(fi, kind, P, N, (kind, D, "refine", refine), threshold=0.05, refine=refine)
        assert want["refits"] == refine
    mask = np.random.default_rng(D).uniform(size=1000) < 0.6
    want, inl = _check_fit(fi, kind, P, N, (kind, D, "mask"), mask=mask, threshold=0.05)
    assert want["candidates"] == int(mask.sum()) and not inl[~mask].any()


def test_a_refit_that_loses_inliers_and_one_the_radius_limit_ends(fi):
    P, N, planted = SR.planted_sphere()
    want0, _ = _check_fit(fi, "sphere", P, None, "planted, no refit", threshold=0.05, r_min=0.5, r_max=5.0, refine=0)
    want2, _ = _check_fit(fi, "sphere", P, None, "planted", threshold=0.05, r_min=0.5, r_max=5.0)
    assert want2["refits"] == 2 and want2["inliers"] < want0["inliers"]
    # the best hypothesis has a radius above 2.003, the least-squares sphere of its inliers one below: the model stays
    held, _ = _check_fit(fi, "sphere", P, None, "r_min ends the refits", threshold=0.05, r_min=2.003, r_max=5.0)
    assert held["found"] == 1 and held["refits"] == 0 and held["radius"] >= 2.003
    free, _ = _check_fit(fi, "sphere", P, None, "the same without refits", threshold=0.05, r_min=2.003, r_max=5.0, refine=0)
    assert _bits(_doubles(free, 3)) == _bits(_doubles(held, 3))
    P, N, planted = SR.planted_cylinder()
    # the first refit stays below 0.4999, the second would not: it is skipped, and the model is that of one refit
    held, _ = _check_fit(fi, "cylinder", P, N, "r_max ends the refits", threshold=0.05, r_min=0.1, r_max=0.4999)
    assert held["found"] == 1 and held["refits"] == 1 and held["radius"] <= 0.4999
    once, _ = _check_fit(fi, "cylinder", P, N, "one refit", threshold=0.05, r_min=0.1, r_max=0.4999, refine=1)
    assert _bits(_doubles(once, 3)) == _bits(_doubles(held, 3))


@pytest.mark.parametrize("kind,D", MODELS)
def test_non_finite_points_unusable_normals_and_duplicates(fi, kind, D):
    P, N = SR.shape_cloud(31 + D, 1000, 0.5, KIND[kind], D)
    P[::7, 1] = np.nan
    P[3::50, 0] = np.inf
    P[5::90, D - 1] = -np.inf
    finite = np.isfinite(P).all(axis=1)
    want, inl = _check_fit(fi, kind, P, N if kind == "cylinder" else None, (kind, D, "non-finite"), threshold=0.05)
    assert want["candidates"] == int(finite.sum()) and not inl[~finite].any()
    N[1::11] = 0.0
    N[2::13, 0] = np.nan
    N[4::17, D - 1] = np.inf
    usable = finite & np.isfinite(N).all(axis=1) & (N != 0).any(axis=1)
    want, inl = _check_fit(fi, kind, P, N, (kind, D, "normals"), threshold=0.05)
    assert want["found"] == 1 and want["candidates"] == int(usable.sum()) and not inl[~usable].any()
    _check_segment(fi, kind, P, N, 2, (kind, D, "segment"), threshold=0.05)
    # one point seventy times: every draw coincides in space, no radius and no axis
    want, _ = _check_fit(fi, kind, np.repeat(P[1:2], 70, axis=0), np.repeat(N[:1], 70, axis=0), (kind, D, "duplicates"), threshold=0.05,
                         max_trials=200)
    assert (want["found"], want["candidates"], want["trials"]) == (0, 70, 200)


@pytest.mark.parametrize("kind,D,radius", [("sphere", 3, 2.0), ("sphere", 2, 2.0), ("cylinder", 3, 1.0)])
def test_radius_limits_on_both_sides(fi, kind, D, radius):
    P, N = _cloud(kind, D, 40 + D, 1000, 0.5)
    near, _ = _check_fit(fi, kind, P, N, (kind, D, "around"), threshold=0.05, r_min=radius - 0.1, r_max=radius + 0.1)
    assert abs(near["radius"] - radius) < 0.05 and near["inliers"] >= 480
    for name, lim in (("below", dict(r_min=0.0, r_max=radius - 0.2)), ("above", dict(r_min=radius + 0.2, r_max=math.inf)),
                      ("above, bounded", dict(r_min=radius + 0.2, r_max=4 * radius))):
        want, _ = _check_fit(fi, kind, P, N, (kind, D, name), threshold=0.05, **lim)
        assert want["inliers"] < 250 and (not want["found"] or lim["r_min"] <= want["radius"] <= lim["r_max"])
    none, _ = _check_fit(fi, kind, P, N, (kind, D, "no radius fits"), threshold=0.05, r_min=1000.0, r_max=1000.5)
    assert none["found"] == 0 and none["trials"] == 1024


@pytest.mark.parametrize("kind,D", MODELS)
def test_the_angle_test(fi, kind, D):
    P, N = SR.shape_cloud(50 + D, 1000, 0.5, KIND[kind], D)
    # a fifth of the shape's own points get a random normal: in the band, but facing elsewhere
    rng = np.random.default_rng(D)
    turned = rng.uniform(size=1000) < 0.2
    N[turned] = rng.normal(size=(int(turned.sum()), D)).astype(np.float32)
    free, _ = _check_fit(fi, kind, P, N, (kind, D, "normal_cos 0"), threshold=0.05, max_angle=None)
    held, inl = _check_fit(fi, kind, P, N, (kind, D, "20 degrees"), threshold=0.05, max_angle=20.0)
    assert held["found"] == 1 and held["candidates"] == free["candidates"] == 1000 and 300 <= held["inliers"] < free["inliers"]
    assert _cos(20.0) == COS20
    _check_segment(fi, kind, P, N, 2, (kind, D, "segment, 20 degrees"), threshold=0.05, max_angle=20.0, min_inliers=50)


@pytest.mark.parametrize("D", [3, 2])
def test_a_sphere_with_normals_that_are_not_tested_is_the_sphere_without(fi, D):
    P, N = SR.shape_cloud(60 + D, 1000, 0.5, SR.SPHERE, D)
    plain, plain_inl = _check_fit(fi, "sphere", P, None, (D, "no normals"), threshold=0.05)
    given, given_inl = _check_fit(fi, "sphere", P, N, (D, "normals"), threshold=0.05)
    assert np.array_equal(plain_inl, given_inl) and [plain[k] for k in INTS] == [given[k] for k in INTS]
    assert _bits(_doubles(plain, D)) == _bits(_doubles(given, D))
    # normals that drop points do what a mask of the usable points does, in every bit
    N[::9] = 0.0
    usable = (N != 0).any(axis=1)
    fewer, fewer_inl = _check_fit(fi, "sphere", P, N, (D, "dropped"), threshold=0.05)
    masked, masked_inl = _check_fit(fi, "sphere", P, None, (D, "masked"), threshold=0.05, mask=usable)
    assert fewer["candidates"] == int(usable.sum()) < plain["candidates"]
    assert np.array_equal(fewer_inl, masked_inl) and [fewer[k] for k in INTS] == [masked[k] for k in INTS]
    assert _bits(_doubles(fewer, D)) == _bits(_doubles(masked, D))


def _two(kind, D):
    """two shapes of 700 and 300 points in 200 strays"""
    rng = np.random.default_rng(5 + D)
    if kind == "sphere":
        a, na = SR.sphere_part(rng, 700, [2.5, 2.5, 2.5], 2.0, 0.02, D)
        b, nb = SR.sphere_part(rng, 300, [7.0, 6.0, 7.0], 1.0, 0.02, D)
    else:
        a, na = SR.cylinder_part(rng, 700, [2.5, 2.5, 4.0], [0.1, 0.2, 1.0], 1.0, 6.0, 0.02, 0.02)
        b, nb = SR.cylinder_part(rng, 300, [7.0, 6.0, 4.0], [1.0, 0.3, 0.1], 0.5, 4.0, 0.02, 0.02)
    P = np.concatenate([a, b, rng.uniform(0.0, 9.0, (200, D))])
    N = np.concatenate([na, nb, rng.normal(size=(200, D))])
    perm = rng.permutation(len(P))
    return np.ascontiguousarray(P[perm], np.float32), np.ascontiguousarray(N[perm], np.float32)


@pytest.mark.parametrize("kind,D", MODELS)
def test_two_shapes_peeled_off(fi, kind, D):
    P, N = _two(kind, D)
    N = N if kind == "cylinder" else None
    labels, models = _check_segment(fi, kind, P, N, 3, (kind, D, "two"), threshold=0.05, min_inliers=250, seed=2 ** 64 - 1)   # the seed wraps
    assert len(models) == 2 and models[0]["inliers"] >= 700 and 300 <= models[1]["inliers"] < 400
    labels, models = _check_segment(fi, kind, P, N, 3, (kind, D, "the second is cut"), threshold=0.05, min_inliers=500, seed=2 ** 64 - 1)
    assert len(models) == 1 and set(labels.tolist()) == {-1, 0}
    _check_segment(fi, kind, P, N, 1, (kind, D, "one asked for"), threshold=0.05, mask=np.arange(len(P)) % 3 != 0)


def test_the_planted_scenes(fi):
    P, N, planted = SR.planted_sphere()
    want, inl = _check_fit(fi, "sphere", P, None, "scene (a)", threshold=0.05, r_min=0.5, r_max=5.0)
    assert want["found"] == 1 and inl[planted].sum() >= 0.95 * planted.sum() and inl[~planted].sum() <= 0.05 * inl.sum()
    P, N, planted = SR.planted_cylinder()
    want, inl = _check_fit(fi, "cylinder", P, N, "scene (b)", threshold=0.05, r_min=0.1, r_max=2.0)
    assert want["found"] == 1 and inl[planted].sum() >= 0.95 * planted.sum() and inl[~planted].sum() <= 0.05 * inl.sum()
    empty = np.zeros((0, 3), np.float32)
    model, inl = fi.segment_sphere(empty, 0.1)
    assert not model["found"] and inl.shape == (0,)
    model, inl = fi.segment_cylinder(empty, empty, 0.1)
    assert not model["found"] and inl.shape == (0,) and not model["axis"].any()
    labels, models = fi.segment_shapes(empty, "sphere", 0.1, 2)
    assert models == [] and labels.shape == (0,)


def test_repeated_calls_return_the_same_bytes(fi):
    for kind, D in MODELS:
        P, N = SR.shape_cloud(50, 4099, 0.3, KIND[kind], D)
        first = _raw(kind, P, N, None, max_trials=2048, confidence=0.0, max_angle=20.0)
        seg = _raw(kind, P, N, None, max_shapes=3)
        for _ in range(3):
            again = _raw(kind, P, N, None, max_trials=2048, confidence=0.0, max_angle=20.0)
            assert again[0] == 0 and np.array_equal(again[2], first[2])
            _same_row(again[1], first[1], D, kind)
            more = _raw(kind, P, N, None, max_shapes=3)
            assert np.array_equal(more[2], seg[2]) and len(more[1]) == len(seg[1])
            for g, w in zip(more[1], seg[1]):
                _same_row(g, w, D, kind)


def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    P, N = SR.shape_cloud(1, 25, 0.5, SR.CYLINDER, 3)
    INVALID, UNSUPPORTED = 1, 5
    bad = [dict(threshold=-1.0), dict(threshold=math.nan), dict(threshold=math.inf), dict(max_trials=0), dict(max_trials=2 ** 20 + 1),
           dict(confidence=1.0), dict(confidence=-0.5), dict(confidence=math.nan), dict(refine=-1), dict(refine=17),
           dict(memory=2), dict(ndim=1), dict(ndim=4), dict(code_of_kind=2), dict(code_of_kind=-1), dict(r_min=-0.5), dict(r_min=2.0, r_max=1.0),
           dict(r_min=math.nan), dict(r_max=math.nan), dict(r_max=-math.inf)]
    for kw in bad:
        for kind in ("sphere", "cylinder"):
            for shapes in (None, 2):
                assert _raw(kind, P, N, None, max_shapes=shapes, **kw)[0] == INVALID, (kind, kw)
    for shapes in (None, 2):
        assert _raw("cylinder", P, None, None, max_shapes=shapes)[0] == INVALID                      # a cylinder without normals
        assert _raw("cylinder", P[:, :2], N[:, :2], None, max_shapes=shapes)[0] == UNSUPPORTED      # a cylinder in 2-D
        assert _raw("sphere", P, None, None, max_shapes=shapes, max_angle=20.0)[0] == INVALID        # normal_cos > 0 without normals
        assert _raw("sphere", P, N, None, max_shapes=shapes, max_angle=20.0)[0] == 0
        assert _raw("sphere", P, None, None, max_shapes=shapes, r_min=1.0, r_max=1.0)[0] == 0        # an interval of one radius
        assert _raw("sphere", P, None, None, max_shapes=shapes, r_max=math.inf)[0] == 0
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    model, rows, found = _capi.FiShapeModel(), (_capi.FiShapeModel * 2)(), C.c_int(0)
    labels = np.empty(25, np.int32)
    for cos, code in ((1.5, INVALID), (-0.5, INVALID), (math.nan, INVALID), (0.5, 0), (1.0, 0)):
        opt = _capi.FiShapeOptions(0, 0.1, 0.0, math.inf, cos, 100, 0.9, 0, 0)
        assert L.fi_shape_fit(3, 25, ptr(P), ptr(N), None, C.byref(opt), C.byref(model), None, 0) == code, cos
    opt = _capi.FiShapeOptions(0, 0.1, 0.0, math.inf, 0.0, 100, 0.9, 0, 0)
    assert L.fi_shape_fit(3, 25, ptr(P), None, None, C.byref(opt), C.byref(model), None, 0) == 0      # inliers may be NULL
    assert L.fi_shape_fit(3, 25, None, None, None, C.byref(opt), C.byref(model), None, 0) == INVALID
    assert L.fi_shape_fit(3, 25, ptr(P), None, None, None, C.byref(model), None, 0) == INVALID
    assert L.fi_shape_fit(3, 25, ptr(P), None, None, C.byref(opt), None, None, 0) == INVALID
    assert L.fi_shape_fit(3, -1, ptr(P), None, None, C.byref(opt), C.byref(model), None, 0) == INVALID
    assert L.fi_shape_fit(3, 2 ** 31, ptr(P), None, None, C.byref(opt), C.byref(model), None, 0) == UNSUPPORTED
    seg = lambda **kw: L.fi_shapes_segment(3, kw.get("n", 25), ptr(P), None, None, C.byref(opt), kw.get("shapes", 2), kw.get("least", 0),  # noqa: E731
                                           kw.get("labels", ptr(labels)), kw.get("rows", rows), kw.get("found", C.byref(found)), 0)
    assert seg() == 0
    assert seg(shapes=0) == INVALID and seg(least=-1) == INVALID and seg(labels=None) == INVALID and seg(rows=None) == INVALID
    assert seg(found=None) == INVALID and seg(n=-1) == INVALID and seg(n=2 ** 31) == UNSUPPORTED
    assert b"points" in L.fi_last_error()
    with pytest.raises(_capi.FiError):
        fi.segment_sphere(P, -1.0)
    with pytest.raises(_capi.FiError):
        fi.segment_shapes(P[:, :2], "cylinder", 0.1, 2, normals=N[:, :2])
    for call in (lambda: fi.segment_sphere(P.reshape(-1), 0.1), lambda: fi.segment_cylinder(P, None, 0.1),
                 lambda: fi.segment_sphere(P, 0.1, max_angle=20.0), lambda: fi.segment_sphere(P, 0.1, normals=N[:20]),
                 lambda: fi.segment_shapes(P, "cone", 0.1, 2), lambda: fi.segment_sphere(P, 0.1, normals=N, max_angle=90.0)):
        with pytest.raises(ValueError):
            call()


def test_device_tensors(tmp_path):
    """the same answers from torch tensors that stay on the device, checked in a fresh process (tests/shape_torch_worker.py),
    as torch must stay out of this one"""
    P, N, planted = SR.planted_cylinder()
    mask = np.arange(len(P)) % 5 != 0
    np.savez(tmp_path / "in.npz", pos=P, nrm=N, mask=mask)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shape_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"].all()
    want, inl = SR.fit(P, SR.CYLINDER, 0.05, 0.1, 2.0, normals=N, mask=mask)
    assert np.array_equal(o["cyl_inliers"], inl.astype(bool))
    assert o["cyl_ints"].tolist() == [want[k] for k in INTS] and _bits(o["cyl_doubles"]) == _bits(_doubles(want, 3))
    want, inl = SR.fit(P, SR.SPHERE, 0.05, 0.5, 5.0, normals=N, normal_cos=COS20)
    assert np.array_equal(o["sph_inliers"], inl.astype(bool))
    assert o["sph_ints"].tolist() == [want[k] for k in INTS] and _bits(o["sph_doubles"]) == _bits(_doubles(want, 3)[:5])
    labels, models = SR.segment(P, SR.CYLINDER, 0.05, 2, min_inliers=500, r_min=0.1, r_max=2.0, normals=N)
    assert np.array_equal(o["labels"], labels) and o["labels"].dtype == np.int32 and int(o["shapes"]) == len(models)
