"""Plane segmentation on the device (fi_plane.hip through segment_plane, segment_planes and the raw fi_plane_fit /
fi_planes_segment) against the numpy restatement of the contract (tests/plane_reference.py): inlier masks and labels
array-equal, every integer of a model equal and every double as a bit pattern.  2- and 3-D, the sizes where a tile of the
score, a chunk of the tree sums and a wave end, trial counts on both sides of a batch, inlier shares of a tenth, a half and
all, refits, a mask, an axis constraint, the cases of tests/test_plane_reference.py with answers known by hand, duplicates,
non-finite points, a refit that loses inliers, the stop rule over several batches, the cube, repeated calls, the error codes,
clean_points with and without remove_planes, and device tensors through a child process."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import plane_reference as PR
from test_plane_reference import cube_faces, grid_plane, off_points

pytestmark = pytest.mark.gpu

COUNTS = [2, 3, 63, 64, 65, 255, 256, 257, 1000, 4099]     # both sides of a wave (64), of a tile and a chunk (256); 17 chunks
MANY = [16384, 16385]                                       # all inliers: 64 chunks, one load of the ordered sum, and a 65th
TRIALS = [1, 1023, 1024, 1025, 3000]                       # both sides of a batch (1024), two batches and a partial one
SHARES = [0.1, 0.5, 1.0]
INTS = ("found", "refits", "inliers", "candidates", "trials")


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist()


def _same_model(got, want, D, what=""):
    """got: segment_plane's dict; want: the restatement's"""
    for key in INTS:
        assert int(got[key]) == int(want[key]), (what, key, got, want)
    assert got["normal"].dtype == np.float64 and got["normal"].shape == (D,), what
    assert _bits(got["normal"]) == _bits(want["normal"][:D]), (what, got, want)
    assert _bits(got["offset"]) == _bits(want["offset"]) and _bits(got["rms"]) == _bits(want["rms"]), (what, got, want)


def _min_cos(max_angle):
    return 0.0 if max_angle is None else float(np.float32(math.cos(math.radians(max_angle))))


def _raw(P, mask, max_planes=None, min_inliers=0, threshold=0.1, max_trials=1024, confidence=0.999, refine=2, seed=0, axis=None,
         max_angle=None, ndim=None, memory=0):
    """the C entries with host buffers -> (code, model dict or list of them, inliers or labels)"""
    from field_interpolation_amd import _capi
    from field_interpolation_amd.api import _plane_dict
    L = _capi.lib()
    P = np.ascontiguousarray(P, np.float32)
    n, D = P.shape[0], (P.shape[1] if ndim is None else ndim)
    opt = _capi.FiPlaneOptions(threshold, max_trials, confidence, refine, seed)
    if axis is not None:
        opt.axis[:len(axis)] = list(axis)
        opt.min_cos = _min_cos(max_angle)
    mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    if max_planes is None:
        model, inl = _capi.FiPlaneModel(), np.full(n, 7, np.uint8)
        code = L.fi_plane_fit(D, n, ptr(P), ptr(mk), C.byref(opt), C.byref(model), ptr(inl), memory)
        return code, _plane_dict(model, D), inl
    rows, labels, found = (_capi.FiPlaneModel * max(max_planes, 1))(), np.full(n, 7, np.int32), C.c_int(-1)
    code = L.fi_planes_segment(D, n, ptr(P), ptr(mk), C.byref(opt), max_planes, min_inliers, ptr(labels), rows, C.byref(found), memory)
    return code, [_plane_dict(rows[i], D) for i in range(max(found.value, 0))], labels


def _check_fit(fi, P, what="", mask=None, max_angle=None, **kw):
    """segment_plane and the raw entry against the restatement"""
    D = P.shape[1]
    want, want_inl = PR.fit(P, mask=mask, min_cos=_min_cos(max_angle), **kw)
    model, inl = fi.segment_plane(P, mask=mask, max_angle=max_angle, **kw)
    assert inl.dtype == np.bool_ and np.array_equal(inl, want_inl.astype(bool)), (what, np.flatnonzero(inl != want_inl.astype(bool))[:5])
    _same_model(model, want, D, what)
    code, model, inl = _raw(P, mask, max_angle=max_angle, **kw)
    assert code == 0 and np.array_equal(inl, want_inl), what
    _same_model(model, want, D, what)
    return want, want_inl


def _check_segment(fi, P, max_planes, what="", mask=None, max_angle=None, **kw):
    D = P.shape[1]
    want_labels, want = PR.segment(P, max_planes=max_planes, mask=mask, min_cos=_min_cos(max_angle), **kw)
    labels, models = fi.segment_planes(P, max_planes=max_planes, mask=mask, max_angle=max_angle, **kw)
    assert labels.dtype == np.int32 and np.array_equal(labels, want_labels), what
    code, rows, raw_labels = _raw(P, mask, max_planes=max_planes, max_angle=max_angle, **kw)
    assert code == 0 and np.array_equal(raw_labels, want_labels), what
    for got in (models, rows):
        assert len(got) == len(want), (what, len(got), len(want))
        for g, w in zip(got, want):
            _same_model(g, w, D, what)
    return want_labels, want


@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("D", [2, 3])
def test_sizes(fi, D, share):
    for n in COUNTS + (MANY if share == 1.0 else []):
        P = PR.plane_cloud(100 * D + n, n, share, D)
        want, _ = _check_fit(fi, P, (D, n, share), threshold=0.1, max_trials=1025, refine=1, seed=n)
        assert want["found"] == (1 if n >= D else 0)
        if n == 16384:
            assert want["inliers"] == 64 * 256
        if n == 16385:
            assert want["inliers"] > 64 * 256


@pytest.mark.parametrize("confidence", [0.0, 0.999])
@pytest.mark.parametrize("D", [2, 3])
def test_trial_counts(fi, D, confidence):
    P = PR.plane_cloud(7 + D, 1000, 0.5, D)
    for trials in TRIALS:
        want, _ = _check_fit(fi, P, (D, trials), threshold=0.1, max_trials=trials, confidence=confidence, seed=3)
        assert want["trials"] == (trials if confidence == 0.0 else min(trials, 1024))


@pytest.mark.parametrize("D", [2, 3])
def test_refits_masks_and_planes(fi, D):
    P = PR.plane_cloud(20 + D, 1000, 0.5, D)
    for refine in (0, 1, 4):
        want, _ = _check_fit(fi, P, (D, "refine", refine), threshold=0.1, refine=refine)
        assert want["refits"] == refine
    rng = np.random.default_rng(D)
    mask = rng.uniform(size=1000) < 0.6
    want, inl = _check_fit(fi, P, (D, "mask"), mask=mask, threshold=0.1)
    assert want["candidates"] == int(mask.sum()) and not inl[~mask].any()
    P2 = np.concatenate([P, PR.plane_cloud(40 + D, 600, 0.7, D)])
    labels, models = _check_segment(fi, P2, 3, (D, "segment"), threshold=0.1, min_inliers=100, seed=2 ** 64 - 1)   # the seed wraps
    assert len(models) >= 2
    _check_segment(fi, P2, 3, (D, "segment, masked"), mask=np.arange(1600) % 3 != 0, threshold=0.1, min_inliers=2000)


def test_an_axis_refuses_the_dominant_plane(fi):
    rng = np.random.default_rng(11)
    floor = np.stack([rng.uniform(0, 31, 500), rng.uniform(0, 31, 500), 4.0 + rng.uniform(-0.04, 0.04, 500)], axis=1)
    wall = np.stack([9.0 + rng.uniform(-0.04, 0.04, 300), rng.uniform(0, 31, 300), rng.uniform(0, 31, 300)], axis=1)
    P = np.concatenate([floor, wall, rng.uniform(0, 31, (200, 3))]).astype(np.float32)[rng.permutation(1000)]
    free, _ = _check_fit(fi, P, "free", threshold=0.1)
    assert free["normal"][2] > 0.99 and free["inliers"] >= 500
    held, _ = _check_fit(fi, P, "held", threshold=0.1, axis=[2.0, 0.0, 0.0], max_angle=20.0)
    assert held["normal"][0] > 0.99 and 300 <= held["inliers"] < 400
    line = PR.plane_cloud(5, 500, 0.6, 2)
    _check_fit(fi, line, "2-D held", threshold=0.1, axis=[0.0, 1.0], max_angle=30.0)
    with pytest.raises(ValueError):
        fi.segment_plane(P, 0.1, axis=[1, 0, 0])


def test_answers_known_by_hand(fi):
    P = np.concatenate([off_points()[:5], grid_plane(), off_points()[5:]])
    for refine in (0, 2):
        model, inl = fi.segment_plane(P, 0.0, refine=refine)
        assert model["normal"].tolist() == [0.0, 0.0, 1.0] and model["offset"] == -3.0 and model["rms"] == 0.0
        assert model["inliers"] == 25 and inl.tolist() == [False] * 5 + [True] * 25 + [False] * 5
        _check_fit(fi, P, "grid", threshold=0.0, refine=refine)
    side = np.float32([[0, 0], [4, 0], [0, 4], [4, 4]])
    P = np.concatenate([grid_plane()] + [np.concatenate([side, np.full((4, 1), z, np.float32)], axis=1) for z in (4.0, 2.0)])
    at = fi.segment_plane(P, 1.0, refine=0, axis=[0, 0, 1], max_angle=0.0)
    below = fi.segment_plane(P, np.nextafter(np.float32(1.0), np.float32(0.0)), refine=0, axis=[0, 0, 1], max_angle=0.0)
    assert at[0]["inliers"] == 33 and below[0]["inliers"] == 25 and below[1].tolist() == [True] * 25 + [False] * 8
    _check_fit(fi, P, "threshold", threshold=1.0, refine=0, axis=[0, 0, 1], max_angle=0.0)
    # nothing to find: collinear points; fewer than D candidates
    line = np.stack([np.arange(20.0), 2.0 * np.arange(20.0), -np.arange(20.0)], axis=1).astype(np.float32)
    want, _ = _check_fit(fi, line, "collinear", threshold=0.1, max_trials=1500)
    assert want["found"] == 0 and want["trials"] == 1500
    few = grid_plane()
    few[3:, 0] = np.nan
    few[1, 1] = np.inf
    want, _ = _check_fit(fi, few, "two finite", threshold=0.1)
    assert (want["found"], want["trials"], want["candidates"]) == (0, 0, 2)
    labels, models = _check_segment(fi, few, 2, "two finite", threshold=0.1)
    assert models == [] and (labels == -1).all()
    empty = np.zeros((0, 3), np.float32)
    model, inl = fi.segment_plane(empty, 0.1)
    assert not model["found"] and inl.shape == (0,)
    labels, models = fi.segment_planes(empty, 0.1, 2)
    assert models == [] and labels.shape == (0,)
    # two parallel planes of sixteen
    P = np.concatenate([grid_plane(0.0, 4), grid_plane(5.0, 4)])[np.random.default_rng(2).permutation(32)]
    want, _ = _check_fit(fi, P, "tie", threshold=0.0, refine=0, seed=7)
    assert want["inliers"] == 16


def test_duplicates_and_non_finite_points(fi):
    P = PR.plane_cloud(31, 600, 0.5, 3)
    P[100:400] = P[np.random.default_rng(9).integers(0, 100, 300)]     # half the cloud copies of a hundred points: equal draws
    _check_fit(fi, P, "duplicates", threshold=0.1)
    _check_fit(fi, np.repeat(P[:1], 70, axis=0), "one point seventy times", threshold=0.1, max_trials=200)
    P = PR.plane_cloud(32, 1000, 0.5, 3)
    P[::7, 1] = np.nan
    P[3::50, 0] = np.inf
    P[5::90, 2] = -np.inf
    want, inl = _check_fit(fi, P, "non-finite", threshold=0.1)
    assert want["candidates"] == int(np.isfinite(P).all(axis=1).sum()) and not inl[~np.isfinite(P).all(axis=1)].any()
    _check_segment(fi, P, 2, "non-finite", threshold=0.1)
    P2 = PR.plane_cloud(33, 300, 1.0, 2)
    P2[::5] = np.nan
    _check_fit(fi, P2, "non-finite 2-D", threshold=0.1)


def test_a_refit_that_loses_inliers_and_the_cut(fi):
    P, floor = PR.planted_cloud()
    want0, _ = _check_fit(fi, P, "planted, no refit", threshold=0.15, refine=0)
    want2, inl = _check_fit(fi, P, "planted", threshold=0.15)
    assert (want0["inliers"], want2["inliers"], want2["refits"]) == (2016, 2015, 2)
    assert inl[floor].all() and int(inl[~floor].sum()) == 15
    # clustering alone has nothing to cut; with the floor gone the largest cluster is the rest of the sphere
    assert fi.cluster_points(P, 1.5).max() == 0
    rng = np.random.default_rng(70)
    nrm = rng.normal(size=P.shape).astype(np.float32)
    val = rng.normal(size=len(P)).astype(np.float32)
    got = fi.clean_points(P, nrm, val, remove_planes=dict(threshold=0.15, max_planes=1), cluster_eps=1.5, largest=1)
    labels, models = fi.segment_planes(P, 0.15, 1)
    rest = labels < 0
    assert int(rest.sum()) == 1485
    for g, w in zip(got[:3], (P[rest], nrm[rest], val[rest])):
        assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), w.view(np.uint32))
    report = got[3]
    assert (report["input"], report["planes"], report["cluster"], report["output"]) == (3500, 2015, 0, 1485)
    assert len(report["plane_models"]) == 1
    _same_model(report["plane_models"][0], want2, 3, "report")
    assert report["clusters"]["clusters"] == 1
    # without remove_planes: what the steps give by hand, as before
    plain = fi.clean_points(P, nrm, val, cluster_eps=1.5, largest=1)
    assert sorted(plain[3]) == ["cluster", "clusters", "input", "output"] and plain[3]["cluster"] == 0 and plain[3]["output"] == 3500
    for g, w in zip(plain[:3], (P, nrm, val)):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    untouched = fi.clean_points(P, nrm, val)
    assert untouched[3] == {"input": 3500, "output": 3500} and untouched[0] is not None and np.array_equal(untouched[0], P)


def test_the_stop_rule_over_several_batches(fi):
    rng = np.random.default_rng(3)
    flat = np.concatenate([rng.uniform(0, 31, (300, 2)), np.full((300, 1), 4.0)], axis=1).astype(np.float32)
    mixed = np.concatenate([flat[:30], rng.uniform(0, 31, (270, 3)).astype(np.float32)])[rng.permutation(300)]
    want, _ = _check_fit(fi, mixed, "several batches", threshold=0.01, max_trials=20000, refine=0)
    assert 1024 < want["trials"] <= 7168
    want, _ = _check_fit(fi, flat, "one batch", threshold=0.01, max_trials=5000)
    assert want["trials"] == 1024


def test_the_cube(fi):
    P, _face = cube_faces()
    labels, models = _check_segment(fi, P, 8, "cube", threshold=0.01, min_inliers=50, max_trials=8192)
    assert len(models) == 6 and (labels >= 0).all()
    for model in models:
        assert sorted(np.abs(model["normal"]).tolist()) == [0.0, 0.0, 1.0]


def test_repeated_calls_return_the_same_bytes(fi):
    P = PR.plane_cloud(50, 4099, 0.3, 3)
    first = _raw(P, None, threshold=0.1, max_trials=2048, confidence=0.0)
    seg = _raw(P, None, max_planes=3, threshold=0.1)
    for _ in range(3):
        again = _raw(P, None, threshold=0.1, max_trials=2048, confidence=0.0)
        assert again[0] == 0 and np.array_equal(again[2], first[2])
        _same_model(again[1], first[1], 3)
        more = _raw(P, None, max_planes=3, threshold=0.1)
        assert np.array_equal(more[2], seg[2]) and len(more[1]) == len(seg[1])
        for g, w in zip(more[1], seg[1]):
            _same_model(g, w, 3)


def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    P = grid_plane()
    INVALID, UNSUPPORTED = 1, 5
    bad = [dict(threshold=-1.0), dict(threshold=math.nan), dict(threshold=math.inf), dict(max_trials=0), dict(max_trials=2 ** 20 + 1),
           dict(confidence=1.0), dict(confidence=-0.5), dict(confidence=math.nan), dict(refine=-1), dict(refine=17),
           dict(memory=2), dict(ndim=1), dict(ndim=4)]
    for kw in bad:
        for planes in (None, 2):
            assert _raw(P, None, max_planes=planes, **kw)[0] == INVALID, kw
    assert _raw(P, None, axis=[0, 0, 0], max_angle=None)[0] == 0                                       # min_cos = 0: the axis is not read
    opt = _capi.FiPlaneOptions(0.1, 100, 0.9, 0, 0)
    model, rows, found = _capi.FiPlaneModel(), (_capi.FiPlaneModel * 2)(), C.c_int(0)
    labels = np.empty(25, np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for min_cos, axis, code in ((1.5, [0, 0, 1], INVALID), (-0.5, [0, 0, 1], INVALID), (math.nan, [0, 0, 1], INVALID),
                                (0.5, [0, 0, 0], INVALID), (0.5, [math.inf, 0, 1], INVALID), (0.5, [0, math.nan, 1], INVALID),
                                (0.5, [0, 0, 1], 0), (1.0, [0, 0, 1], 0)):
        held = _capi.FiPlaneOptions(0.1, 100, 0.9, 0, 0)
        held.axis[:] = axis
        held.min_cos = min_cos
        assert L.fi_plane_fit(3, 25, ptr(P), None, C.byref(held), C.byref(model), None, 0) == code, (min_cos, axis)
    assert L.fi_plane_fit(3, 25, ptr(P), None, C.byref(opt), C.byref(model), None, 0) == 0            # inliers may be NULL
    assert L.fi_plane_fit(3, 25, None, None, C.byref(opt), C.byref(model), None, 0) == INVALID
    assert L.fi_plane_fit(3, 25, ptr(P), None, None, C.byref(model), None, 0) == INVALID
    assert L.fi_plane_fit(3, 25, ptr(P), None, C.byref(opt), None, None, 0) == INVALID
    assert L.fi_plane_fit(3, -1, ptr(P), None, C.byref(opt), C.byref(model), None, 0) == INVALID
    assert L.fi_plane_fit(3, 2 ** 31, ptr(P), None, C.byref(opt), C.byref(model), None, 0) == UNSUPPORTED
    seg = lambda **kw: L.fi_planes_segment(3, kw.get("n", 25), ptr(P), None, C.byref(opt), kw.get("planes", 2), kw.get("least", 0),  # noqa: E731
                                           kw.get("labels", ptr(labels)), kw.get("rows", rows), kw.get("found", C.byref(found)), 0)
    assert seg() == 0
    assert seg(planes=0) == INVALID and seg(least=-1) == INVALID and seg(labels=None) == INVALID and seg(rows=None) == INVALID
    assert seg(found=None) == INVALID and seg(n=-1) == INVALID and seg(n=2 ** 31) == UNSUPPORTED
    assert b"points" in L.fi_last_error()
    with pytest.raises(_capi.FiError):
        fi.segment_plane(P, -1.0)
    with pytest.raises(ValueError):
        fi.segment_plane(P.reshape(-1), 0.1)


def test_device_tensors(tmp_path):
    """the same answers from torch tensors that stay on the device, checked in a fresh process (tests/plane_torch_worker.py),
    as torch must stay out of this one"""
    P, floor = PR.planted_cloud()
    mask = np.arange(len(P)) % 5 != 0
    np.savez(tmp_path / "in.npz", pos=P, mask=mask)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plane_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"].all()
    want, inl = PR.fit(P, 0.15, mask=mask)
    assert np.array_equal(o["inliers"], inl.astype(bool))
    assert o["ints"].tolist() == [want[k] for k in INTS]
    assert _bits(o["doubles"]) == _bits(list(want["normal"]) + [want["offset"], want["rms"]])
    labels, models = PR.segment(P, 0.15, 2, min_inliers=500)
    assert np.array_equal(o["labels"], labels) and o["labels"].dtype == np.int32 and int(o["planes"]) == len(models) == 1
    assert np.array_equal(o["clean_pos"].view(np.uint32), P[labels < 0].view(np.uint32))
