"""Descriptors and their matching on the device (fi_feature.hip through PointIndex.describe, match_features and the raw
fi_points_describe / fi_feature_match) against the numpy restatement of the contract (tests/feature_reference.py): every
float as a bit pattern, every index and mask equal.  The point counts where a wave and a workgroup end, every list length that
takes another path of the neighbour search, a max_distance that empties lists, points and normals that are not finite, zero
and unnormalised normals, forty copies of one point, a list without the point itself (32 counted pairs), the cases of tests/test_feature_reference.py with answers known by hand;
row widths and counts on both sides of a tile, ties, masks, rows that are not finite, an empty set; repeated calls, the error
codes, and device tensors through a child process (tests/align_torch_worker.py)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import feature_reference as FR
import normals_reference as N
from test_feature_reference import bumpy_cloud, crowd, flat_grid

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 33, 63, 64, 65, 255, 256, 257, 1000, 4099]
KS = [1, 3, 8, 9, 16, 17, 32]


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def scan(n, seed):
    """n points of a wavy sheet with normals near +z that are not unit vectors"""
    rng = np.random.default_rng(seed)
    side = max(2.0, math.sqrt(n) / 2.0)
    x, y = rng.uniform(0, side, n), rng.uniform(0, side, n)
    P = np.stack([x, y, np.sin(x) + 0.5 * np.cos(1.7 * y)], axis=1).astype(np.float32)
    nrm = np.stack([-np.cos(x), 0.85 * np.sin(1.7 * y), np.ones(n)], axis=1) * rng.uniform(0.5, 2.0, (n, 1))
    return P, nrm.astype(np.float32)


def _same_floats(got, want, what=""):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    diff = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert diff.size == 0, (what, diff[:5], got.ravel()[diff[:5]], want.ravel()[diff[:5]])


def _describe_raw(index, nrm, k, max_distance=math.inf, memory=0, **over):
    from field_interpolation_amd import _capi
    n = index.num_points
    nrm = np.ascontiguousarray(nrm, np.float32)
    feat, valid = np.full((n, 33), 7.0, np.float32), np.full(n, 7, np.uint8)
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None  # noqa: E731
    args = dict(h=index._h, normals=ptr(nrm), feat=ptr(feat), valid=ptr(valid))
    args.update(over)
    code = _capi.lib().fi_points_describe(args["h"], args["normals"], k, max_distance, args["feat"], args["valid"], memory)
    return code, feat, valid


def _check_describe(fi, P, nrm, k, max_distance=math.inf, neighbours=None, what=""):
    want, want_valid = FR.describe(P, nrm, k, max_distance, neighbours=neighbours)
    index = fi.PointIndex(P)
    feat, valid = index.describe(nrm, k, max_distance)
    assert valid.dtype == np.bool_ and np.array_equal(valid, want_valid.astype(bool)), (what, np.flatnonzero(valid != want_valid.astype(bool))[:5])
    _same_floats(feat, want, what)
    code, feat, valid = _describe_raw(index, nrm, k, max_distance)
    assert code == 0 and np.array_equal(valid, want_valid), what
    _same_floats(feat, want, what)
    return want, want_valid


@pytest.mark.parametrize("n", COUNTS)
def test_describe_sizes_and_list_lengths(fi, n):
    P, nrm = scan(n, n)
    _, idx = N.knn(P, P, 3, 32)                                            # a list of k is the first k of the list of 32
    for k in KS:
        want, valid = _check_describe(fi, P, nrm, k, neighbours=idx[:, :k], what=(n, k))
        if n >= 33 and k >= 8:
            assert valid.mean() > 0.9, (n, k)


def test_describe_a_max_distance_that_empties_lists(fi):
    P, nrm = scan(1000, 5)
    P[::50, 2] += 40 + 10 * np.arange(20, dtype=np.float32)                # twenty points far from everything and each other
    want, valid = _check_describe(fi, P, nrm, 16, max_distance=1.5, what="max_distance")
    assert not valid[::50].any() and valid.sum() > 900
    _check_describe(fi, P, nrm, 16, max_distance=0.0, what="max_distance 0")


def test_describe_points_and_normals_that_are_not_live(fi):
    P, nrm = scan(1000, 6)
    P[::31, 1], P[5::67, 0] = np.nan, np.inf
    nrm[3::29] = 0.0
    nrm[7::43, 2], nrm[11::47, 0], nrm[13::53, 1] = np.nan, np.inf, -np.inf
    nrm[::3] *= np.float32(1e-20)                                          # tiny but not zero: still a direction
    nrm[1::3] *= np.float32(1e15)
    for k in (8, 32):
        want, valid = _check_describe(fi, P, nrm, k, what=("holes", k))
        dead = ~np.isfinite(P).all(axis=1) | ~np.isfinite(nrm).all(axis=1) | ~nrm.any(axis=1)
        assert not valid[dead].any() and valid[~dead].all()
    # a normal whose length overflows fp32 but not fp64
    nrm[1::3] = np.float32(3e38)
    _check_describe(fi, P, nrm, 8, what="huge normals")


def test_describe_duplicates(fi):
    P, nrm = bumpy_cloud(300)
    D = np.concatenate([np.repeat(P[:1], 40, axis=0), P[20:]])
    dn = np.concatenate([np.repeat(nrm[:1], 40, axis=0), nrm[20:]])
    perm = np.random.default_rng(1).permutation(len(D))
    for k in (16, 32):
        want, valid = _check_describe(fi, D[perm], dn[perm], k, what=("forty copies", k))
        assert int((~valid).sum()) >= 33
    _check_describe(fi, np.repeat(P[:1], 70, axis=0), np.repeat(nrm[:1], 70, axis=0), 8, what="one point seventy times")


def test_describe_a_list_without_the_point_itself(fi):
    """points 1e-30 apart: the search's fp32 distances are 0, the points from 32 on are not in their own lists and count all
    32 pairs in one bin, where a packed 5-bit counter carries"""
    for n in (33, 34, 70):
        P, nrm = crowd(n)
        want, valid = _check_describe(fi, P, nrm, 32, what=("crowd", n))
        assert valid.all()
        _check_describe(fi, P, np.tile(np.float32([1, 0, 1]), (n, 1)), 32, what=("crowd, tilted", n))
        _check_describe(fi, P, np.tile(np.float32([-1, 0, 1]), (n, 1)), 32, what=("crowd, tilted back", n))
        _check_describe(fi, P, nrm, 31, what=("crowd, k = 31", n))


def test_describe_answers_known_by_hand(fi):
    P, nrm = flat_grid()
    want, valid = _check_describe(fi, P, nrm, 9, what="grid")
    feat, _ = fi.PointIndex(P).describe(nrm, 9)
    inner = np.flatnonzero((P[:, 0] > 0) & (P[:, 0] < 8) & (P[:, 1] > 0) & (P[:, 1] < 8))
    assert (feat[inner][:, [5, 16, 27]] == 100.0).all() and (np.delete(feat, [5, 16, 27], axis=1) == 0).all()
    P, nrm = bumpy_cloud()
    Q = np.stack([-P[:, 1], P[:, 0], P[:, 2]], axis=1) + np.float32([5, -3, 4])
    qn = np.stack([-nrm[:, 1], nrm[:, 0], nrm[:, 2]], axis=1)
    a, _ = fi.PointIndex(P).describe(nrm, 32)
    b, _ = fi.PointIndex(Q).describe(qn, 32)
    _same_floats(a, b, "a quarter turn")
    _check_describe(fi, P, nrm, 32, what="bumpy")
    two = np.float32([[0, 0, 0], [0, 0, 2]])
    want, valid = _check_describe(fi, two, np.float32([[0, 0, 1], [0, 0, -3]]), 4, what="along the line")
    assert not valid.any()
    feat, valid = fi.PointIndex(np.zeros((0, 3), np.float32)).describe(np.zeros((0, 3), np.float32))
    assert feat.shape == (0, 33) and valid.shape == (0,)


# ---- matching --------------------------------------------------------------------------------------------------------------

def _match_raw(a, b, va=None, vb=None, dim=None, memory=0, **over):
    from field_interpolation_amd import _capi
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    dim = a.shape[1] if dim is None else dim
    idx, dist = np.full(len(a), 7, np.int64), np.full(len(a), 7.0, np.float32)
    ptr = lambda x: None if x is None or not x.size else C.c_void_p(x.ctypes.data)  # noqa: E731
    va = None if va is None else np.ascontiguousarray(va, np.uint8)
    vb = None if vb is None else np.ascontiguousarray(vb, np.uint8)
    args = dict(na=len(a), pa=ptr(a), pva=ptr(va), nb=len(b), pb=ptr(b), pvb=ptr(vb), idx=ptr(idx), dist=ptr(dist))
    args.update(over)
    code = _capi.lib().fi_feature_match(dim, args["na"], args["pa"], args["pva"], args["nb"], args["pb"], args["pvb"], args["idx"], args["dist"],
                                        memory)
    return code, idx, dist


def _check_match(fi, a, b, va=None, vb=None, what=""):
    want, want_dist = FR.match(a, b, va, vb)
    idx, dist = fi.match_features(a, b, va, vb, distances=True)
    assert idx.dtype == np.int64 and np.array_equal(idx, want), (what, np.flatnonzero(idx != want)[:5])
    _same_floats(dist, want_dist, what)
    assert np.array_equal(fi.match_features(a, b, va, vb), want), what
    code, idx, dist = _match_raw(a, b, va, vb)
    assert code == 0 and np.array_equal(idx, want), what
    _same_floats(dist, want_dist, what)
    return want


def rows(n, dim, seed):
    """n rows on a coarse lattice, so that equal distances are common"""
    return np.random.default_rng(seed).integers(0, 4, (n, dim)).astype(np.float32)


@pytest.mark.parametrize("dim", [1, 33, 64])
def test_match_widths_and_counts(fi, dim):
    for na in (255, 256, 257):
        for nb in (255, 256, 257):
            _check_match(fi, rows(na, dim, na), rows(nb, dim, 1000 + nb), what=(dim, na, nb))
    _check_match(fi, rows(1, dim, 1), rows(1000, dim, 2), what=(dim, 1, 1000))
    _check_match(fi, rows(1000, dim, 3), rows(1, dim, 4), what=(dim, 1000, 1))
    rng = np.random.default_rng(dim)
    _check_match(fi, rng.normal(size=(300, dim)).astype(np.float32), rng.normal(size=(5000, dim)).astype(np.float32), what=(dim, "normal"))


def test_match_ties_masks_and_rows_that_are_not_finite(fi):
    rng = np.random.default_rng(8)
    for dim in (2, 8, 9, 17, 40, 41):
        a, b = rows(600, dim, dim), rows(700, dim, 50 + dim)
        b[300:600] = b[:300]                                               # planted ties: the lower copy must win
        want = _check_match(fi, a, b, what=(dim, "ties"))
        assert (want < 300).sum() > 0 and not ((want >= 300) & (want < 600)).any()
        va, vb = rng.uniform(size=600) < 0.7, rng.uniform(size=700) < 0.5
        want = _check_match(fi, a, b, va, vb, what=(dim, "masks"))
        assert (want[~va] == -1).all() and vb[want[va]].all()
        a[::7, 0], a[3::11, dim - 1] = np.nan, np.inf
        b[::5, dim - 1], b[2::13, 0] = np.nan, -np.inf
        want = _check_match(fi, a, b, va, vb, what=(dim, "not finite"))
        assert (want[::7] == -1).all() and np.isfinite(b[want[want >= 0]]).all()
        _check_match(fi, a, b, None, np.zeros(700, bool), what=(dim, "nothing valid"))
    big = np.float32([[3e19, 3e19], [1, 1]])                                # a squared difference that overflows: +inf is a distance
    want = _check_match(fi, big, np.float32([[-3e19, 0], [-3e19, 1]]), what="overflow")
    assert want.tolist() == [0, 0]
    # the cases known by hand
    b = np.float32([[0, 0], [2, 0], [2, 0], [5, 5], [np.nan, 0], [0, 2]])
    a = np.float32([[2, 0], [1, 1], [np.inf, 0], [5, 4], [0.5, 0.5]])
    assert fi.match_features(a, b).tolist() == [1, 0, -1, 3, 0]
    want, want_dist = FR.match_mutual(a, b)
    idx, dist = fi.match_features(a, b, mutual=True, distances=True)
    assert idx.tolist() == want.tolist() == [1, -1, -1, 3, 0]
    _same_floats(dist, want_dist, "mutual")
    fs, ft = rows(500, 33, 1), rows(400, 33, 2)
    assert np.array_equal(fi.match_features(fs, ft, mutual=True), FR.match_mutual(fs, ft)[0])


def test_match_an_empty_set(fi):
    a = rows(300, 33, 1)
    idx, dist = fi.match_features(a, np.zeros((0, 33), np.float32), distances=True)
    assert (idx == -1).all() and np.isinf(dist).all() and idx.shape == (300,)
    idx = fi.match_features(np.zeros((0, 33), np.float32), a)
    assert idx.shape == (0,)
    assert fi.match_features(a, np.zeros((0, 33), np.float32), mutual=True).tolist() == [-1] * 300


def test_repeated_calls_return_the_same_bytes(fi):
    P, nrm = scan(4099, 9)
    index = fi.PointIndex(P)
    first = index.describe(nrm, 32)
    other = scan(3000, 10)
    ft, _ = fi.PointIndex(other[0]).describe(other[1], 32)
    match = fi.match_features(first[0], ft, distances=True)
    for _ in range(3):
        again = index.describe(nrm, 32)
        _same_floats(again[0], first[0])
        assert np.array_equal(again[1], first[1])
        fi.segment_plane(P, 0.1)
        fi.register_points(P[:200], other[0], mode="point", max_iterations=2)
        more = fi.match_features(first[0], ft, distances=True)
        assert np.array_equal(more[0], match[0])
        _same_floats(more[1], match[1])


def test_error_codes(fi):
    from field_interpolation_amd import _capi
    INVALID, UNSUPPORTED = 1, 5
    P, nrm = scan(100, 1)
    index = fi.PointIndex(P)
    assert _describe_raw(index, nrm, 8)[0] == 0
    assert _describe_raw(index, nrm, 8, valid=None)[0] == 0                               # valid may be NULL
    for kw in (dict(k=0), dict(k=33), dict(k=8, max_distance=-1.0), dict(k=8, max_distance=math.nan), dict(k=8, memory=2),
               dict(k=8, h=None), dict(k=8, normals=None), dict(k=8, feat=None)):
        assert _describe_raw(index, nrm, **kw)[0] == INVALID, kw
    flat = fi.PointIndex(P[:, :2])
    assert _describe_raw(flat, nrm, 8)[0] == UNSUPPORTED and b"3 dimensions" in _capi.lib().fi_last_error()
    assert _describe_raw(flat, nrm, 0)[0] == INVALID
    with pytest.raises(ValueError):
        index.describe(nrm[:50])
    with pytest.raises(ValueError):
        index.describe(nrm, k=40)
    with pytest.raises(_capi.FiError):
        flat.describe(nrm)
    a, b = rows(10, 4, 1), rows(12, 4, 2)
    assert _match_raw(a, b)[0] == 0 and _match_raw(a, b, dist=None)[0] == 0
    for kw in (dict(dim=0), dict(dim=65), dict(na=-1), dict(nb=-1), dict(pa=None), dict(pb=None), dict(idx=None), dict(memory=2)):
        assert _match_raw(a, b, **kw)[0] == INVALID, kw
    assert _match_raw(a, b, na=2 ** 31)[0] == UNSUPPORTED and _match_raw(a, b, nb=2 ** 31)[0] == UNSUPPORTED
    assert _match_raw(a, b, nb=0, pb=None)[0] == 0 and _match_raw(a, b, na=0, pa=None, idx=None)[0] == 0
    with pytest.raises(ValueError):
        fi.match_features(a, rows(12, 5, 2))
    with pytest.raises(ValueError):
        fi.match_features(a, b, valid_a=np.ones(3, bool))


def test_device_tensors(tmp_path):
    """descriptors and matches from torch tensors that stay on the device, checked in a fresh process
    (tests/align_torch_worker.py), as torch must stay out of this one"""
    import align_reference as AR
    sp, sn, tp, tn, _, _ = AR.planted_scans()
    np.savez(tmp_path / "in.npz", sp=sp, sn=sn, tp=tp, tn=tn)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "align_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"].all()
    fs, vs = FR.describe(sp, sn, 32)
    ft, vt = FR.describe(tp, tn, 32)
    _same_floats(o["features"], fs, "features")
    assert np.array_equal(o["valid"], vs.astype(bool))
    want, want_dist = FR.match(fs, ft, vs, vt)
    assert np.array_equal(o["matches"], want) and np.array_equal(o["mutual"], FR.match_mutual(fs, ft, vs, vt)[0])
    _same_floats(o["distances"], want_dist, "distances")
