"""Moving-least-squares projection on the device (fi_mls.hip through fi_mls_project and fi_points_mls_project) against the
numpy definition of the contract (tests/mls_reference.py): positions, normals and curvature as bit patterns (a NaN matches a
NaN), the order array-equal.  2- and 3-D, both degrees, every k at which the walk's list class or the quadric's six
coefficients change, tests/test_gpu_knn.py's clouds plus an exactly planar one and one with non-finite rows, the set's own
points and external queries, radii that cut the list short or leave a point alone, max_move, guide normals, every output left
out in turn, more queries than one chunk, clean_points(smooth=...), the error codes and host / device buffers."""
import ctypes as C
import math

import numpy as np
import pytest

import mls_reference as M
import normals_reference as R
from test_gpu_knn import CLOUDS, _cloud, _field, _queries

pytestmark = pytest.mark.gpu

KS = [1, 2, 5, 6, 8, 9, 16, 17, 32]      # both sides of the list classes 8 / 16 / 32 and of the quadric's six coefficients
SIZES = {2: [40, 30], 3: [20, 18, 16]}
# a radius that cuts the list short for the larger k and fills it for the smaller ones (by the clouds' densities)
RADIUS = {"random": {2: 1.8, 3: 2.5}, "identical": {2: 1.0, 3: 1.0}, "collinear": {2: 0.2, 3: 0.2}, "cluster": {2: 0.02, 3: 0.02},
          "single": {2: 1.0, 3: 1.0}, "outside": {2: 6.0, 3: 12.0}, "grid ties": {2: 1.5, 3: 1.5}, "planar": {2: 1.5, 3: 1.5},
          "non-finite": {2: 1.8, 3: 2.5}}
KINDS = CLOUDS + ["planar", "non-finite"]


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _bits_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if got.dtype == np.float32:
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    else:
        same = got == want
    bad = np.argwhere(~same)
    assert bad.size == 0, (what, len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])


def _same(got, want, what):
    """(positions, normals, curvature, order) of the device against the definition's"""
    assert len(got) == 4
    for g, w, name in zip(got, want, ("positions", "normals", "curvature", "order")):
        _bits_equal(g, w, (what, name))


def _make(rng, kind, D, n=4000):
    sizes = SIZES[D]
    if kind == "planar":                                      # 3-D: a plane of exact fp32 coordinates; 2-D: a line
        uv = rng.uniform(0, 16, size=(n, D - 1)).astype(np.float32)
        last = np.float32(2.0) + np.float32(0.25) * uv[:, 0] + (np.float32(0.5) * uv[:, 1] if D == 3 else np.float32(0.0))
        return np.concatenate([uv, last[:, None]], axis=1).astype(np.float32)
    if kind == "non-finite":
        pos = _queries(rng, sizes, n, 1.0)
        pos[::7, 0] = np.nan
        pos[3::11, D - 1] = np.inf
        pos[5::13, 0] = -np.inf
        return pos
    return _cloud(rng, kind, sizes, n).reshape(-1, D)


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_matches_the_definition(fi, kind, D, degree):
    rng = np.random.default_rng(100 * D + KINDS.index(kind))
    pos = _make(rng, kind, D)
    radius = RADIUS[kind][D]
    q = np.concatenate([_queries(rng, SIZES[D], 2800), pos[:200] + np.float32(0.01)])     # 3 000 external queries
    if kind == "cluster":
        q[:1500] = (np.float32(2.0) + rng.normal(scale=0.012, size=(1500, D))).astype(np.float32)
    if kind == "non-finite":
        q[::9, 0] = np.nan
        q[4::10, D - 1] = -np.inf
    own_nb = R.knn(pos, pos, D, 32, np.float32(radius))[1]
    ext_nb = R.knn(pos, q, D, 32, np.float32(radius))[1]
    f = _field(fi, SIZES[D], pos)
    pi = fi.PointIndex(pos, ndim=D)
    orders = np.zeros(3, np.int64)
    for k in KS:
        want = M.project(pos, D, None, k, radius, degree, neighbours=own_nb)
        orders += np.bincount(want[3], minlength=3)
        for index in (pi, f):
            _same(index.smooth(k=k, radius=radius, degree=degree, curvature=True, order=True), want, (kind, D, degree, k, "own"))
        want = M.project(pos, D, q, k, radius, degree, neighbours=ext_nb)
        orders += np.bincount(want[3], minlength=3)
        for index in (pi, f):
            _same(index.project(q, k=k, radius=radius, degree=degree, curvature=True, order=True), want,
                  (kind, D, degree, k, "queries"))
    print(kind, D, degree, "orders 0 / 1 / 2:", orders)
    if kind in ("random", "non-finite"):                      # the radius cut lists short and every branch was taken
        m = (own_nb >= 0).sum(axis=1)
        assert m.min() < 16 and m.max() == 32
        assert orders[0] > 0 and orders[1] > 0 and (degree == 1 or orders[2] > 0)
    if kind in ("identical", "single") or (kind == "collinear" and D == 3):
        assert orders[2] == 0                                 # refused the quadric


@pytest.mark.parametrize("D", [2, 3])
def test_a_radius_below_the_nearest_spacing_leaves_every_point_alone(fi, D):
    rng = np.random.default_rng(7 + D)
    pos = _queries(rng, SIZES[D], 3000, 1.0)
    got = fi.PointIndex(pos).smooth(k=8, radius=1e-4, degree=2, curvature=True, order=True)
    want = M.project(pos, D, None, 8, 1e-4, 2)
    _same(got, want, "alone")
    assert np.all(got[3] == 0) and np.array_equal(got[0].view(np.uint32), pos.view(np.uint32))
    assert np.all(got[1] == 0) and np.all(np.isnan(got[2]))


@pytest.mark.parametrize("D", [2, 3])
def test_max_move_and_guide_normals(fi, D):
    rng = np.random.default_rng(11 + D)
    pos = _make(rng, "random", D, 3000)
    radius = RADIUS["random"][D] * 1.5
    pi = fi.PointIndex(pos)
    free = pi.smooth(k=16, radius=radius, order=True)
    guides = -free[1].copy()                                   # every dot negative ...
    guides[::2] = rng.normal(size=guides[::2].shape).astype(np.float32)      # ... or of either sign ...
    guides[::5] = np.nan                                       # ... or not a number
    for mm in (math.inf, 0.05, 0.0):
        want = M.project(pos, D, None, 16, radius, 2, max_move=mm, guide_normals=guides)
        got = pi.smooth(k=16, radius=radius, max_move=mm, normals=guides, curvature=True, order=True)
        _same(got, want, ("guides", mm))
    flipped = (got[1] * free[1]).sum(1) < 0
    assert flipped[1::10][free[2][1::10] > 0].all() and flipped.sum() < len(pos) and not flipped[::5].any()
    moved = np.linalg.norm(pi.smooth(k=16, radius=radius, max_move=0.05)[0].astype(np.float64) - pos, axis=1)
    # (the output's fp32 rounding: half an ulp of a coordinate below 64 is 1.9e-6 an axis, 3.3e-6 in length)
    assert moved.max() <= 0.05 + 4e-6 and (np.linalg.norm(free[0].astype(np.float64) - pos, axis=1) > 0.06).any()
    assert np.array_equal(got[0].view(np.uint32), pos.view(np.uint32))       # max_move = 0: nothing moves
    q = _queries(rng, SIZES[D], 1000)
    gq = rng.normal(size=q.shape).astype(np.float32)
    _same(pi.project(q, k=9, radius=radius, degree=1, max_move=0.5, normals=gq, curvature=True, order=True),
          M.project(pos, D, q, 9, radius, 1, max_move=0.5, guide_normals=gq), "guided queries")


def _c_call(L, fn, handle, D, n, q, k, radius, degree, outs, guides=None, max_move=math.inf, memory=0):
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    return fn(handle, n, ptr(q), k, radius, degree, max_move, ptr(guides), *[ptr(o) for o in outs], memory)


def test_every_output_may_be_left_out_but_not_all(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    rng = np.random.default_rng(13)
    pos = _make(rng, "non-finite", 3, 2000)
    q = _queries(rng, SIZES[3], 700)
    pi = fi.PointIndex(pos)
    f = _field(fi, SIZES[3], pos)
    for fn, handle in ((L.fi_points_mls_project, pi._h), (L.fi_mls_project, f._h)):
        for queries, n in ((None, len(pos)), (q, len(q))):
            want = M.project(pos, 3, queries, 12, 2.5, 2)
            for skip in range(4):
                outs = [np.full((n, 3), 7, np.float32), np.full((n, 3), 7, np.float32), np.full(n, 7, np.float32), np.full(n, 7, np.uint8)]
                outs[skip] = None
                assert _c_call(L, fn, handle, 3, n, queries, 12, 2.5, 2, outs) == 0
                for i in range(4):
                    if i != skip:
                        _bits_equal(outs[i], want[i], (skip, i))
            assert _c_call(L, fn, handle, 3, n, queries, 12, 2.5, 2, [None] * 4) == 1


def test_more_queries_than_one_chunk_and_calls_of_different_sizes(fi):
    # the lists' scratch holds 2^18 points: the second chunk starts in the middle of a work group's worth of queries
    rng = np.random.default_rng(17)
    pos = rng.uniform(0, 8, size=(300, 2)).astype(np.float32)
    pi = fi.PointIndex(pos)
    n = (1 << 18) + 77
    q = rng.uniform(-1, 9, size=(n, 2)).astype(np.float32)
    _same(pi.project(q, k=5, radius=1.5, degree=2, curvature=True, order=True), M.project(pos, 2, q, 5, 1.5, 2), "two chunks")
    for m in (10, 5000, 300):                                  # the same index, calls of different sizes, then its own points
        _same(pi.project(q[:m], k=17, radius=1.0, degree=2, curvature=True, order=True), M.project(pos, 2, q[:m], 17, 1.0, 2), m)
    want = M.project(pos, 2, None, 32, 1.0, 2)
    _same(pi.smooth(k=32, radius=1.0, curvature=True, order=True), want, "own")
    _same(pi.smooth(k=32, radius=1.0, curvature=True, order=True), want, "own, again")


def test_empty_sets_and_queries(fi):
    q = np.ones((5, 3), np.float32)
    empty = fi.PointIndex(np.zeros((0, 3), np.float32))
    pos, nrm, cur, order = empty.project(q, radius=1.0, curvature=True, order=True)
    assert np.array_equal(pos, q) and np.all(nrm == 0) and np.all(np.isnan(cur)) and np.all(order == 0)
    assert empty.smooth(radius=1.0)[0].shape == (0, 3)
    assert fi.PointIndex(q).project(np.zeros((0, 3), np.float32), radius=1.0)[1].shape == (0, 3)
    allbad = np.full((10, 2), np.nan, np.float32)              # no finite point: the bits come back
    allbad[3] = [np.inf, 1.0]
    got = fi.PointIndex(allbad).smooth(radius=1.0, order=True)
    assert np.array_equal(got[0].view(np.uint32), allbad.view(np.uint32)) and np.all(got[2] == 0)


def test_smooth_points_and_clean_points(fi):
    rng = np.random.default_rng(19)
    d = rng.normal(size=(3000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = (10.0 + 8.0 * d + rng.normal(scale=0.05, size=d.shape)).astype(np.float32)
    pos = np.concatenate([pos, rng.uniform(0, 20, size=(60, 3)).astype(np.float32)])     # strays for the outlier rule
    nrm = np.concatenate([d, d[:60]]).astype(np.float32)
    val = rng.normal(size=len(pos)).astype(np.float32)
    args = dict(k=8, std_ratio=1.5, radius=2.0, min_neighbours=3)
    before = fi.clean_points(pos, nrm, val, **args)
    again = fi.clean_points(pos, nrm, val, smooth=None, **args)
    for a, b in zip(before[:3], again[:3]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert "smoothed" not in before[3] and before[3]["output"] < len(pos)
    opts = dict(radius=2.5, k=32, degree=2, max_move=0.3)
    got = fi.clean_points(pos, nrm, val, smooth=opts, **args)
    by_hand = fi.smooth_points(before[0], normals=before[1], order=True, **opts)
    want = M.project(before[0], 3, None, 32, 2.5, 2, max_move=0.3, guide_normals=before[1])
    for g, w in zip(by_hand, (want[0], want[1], want[3])):
        _bits_equal(g, w, "smooth_points")
    assert np.array_equal(got[0].view(np.uint32), by_hand[0].view(np.uint32))
    assert np.array_equal(got[1].view(np.uint32), by_hand[1].view(np.uint32))
    assert np.array_equal(got[2], before[2]) and got[3]["smoothed"] == int((by_hand[2] > 0).sum())
    assert got[3]["output"] == before[3]["output"] and np.array_equal(got[3]["smooth_order"], by_hand[2])
    assert np.all((got[1] * before[1]).sum(1)[by_hand[2] > 0] > 0)            # the given normals' orientation is kept
    no_normals = fi.clean_points(pos, smooth=opts, **args)
    assert no_normals[1] is None and no_normals[0].shape == before[0].shape


def test_device_tensors(tmp_path):
    """torch device tensors in, torch device tensors out, equal to the definition; in a fresh process
    (tests/mls_torch_worker.py), as torch must stay out of this one"""
    import os
    import subprocess
    import sys
    rng = np.random.default_rng(23)
    pos = _make(rng, "random", 3, 3000)
    pos[5] = np.nan
    q = _queries(rng, SIZES[3], 1500)
    g = rng.normal(size=pos.shape).astype(np.float32)
    np.savez(tmp_path / "in.npz", pos=pos, q=q, g=g)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mls_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"].all()
    own = M.project(pos, 3, None, 16, 2.5, 2, max_move=0.5, guide_normals=g)
    ext = M.project(pos, 3, q, 16, 2.5, 1)
    for name in ("pts", "ctx"):
        _same([o["%s_own_%d" % (name, i)] for i in range(4)], own, (name, "own"))
        _same([o["%s_ext_%d" % (name, i)] for i in range(4)], ext, (name, "queries"))
    _same([o["free_%d" % i] for i in range(4)], own, "smooth_points")
    _same([o["mixed_%d" % i] for i in range(4)], own, "host normals, device=True")


def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    pos = np.random.default_rng(29).uniform(0, 9, size=(40, 3)).astype(np.float32)
    f = _field(fi, [10, 10, 10], pos)
    pi = fi.PointIndex(pos)
    out = [np.empty((40, 3), np.float32), None, None, None]
    inf, nan = math.inf, math.nan
    for fn, h in ((L.fi_mls_project, f._h), (L.fi_points_mls_project, pi._h)):
        call = lambda n, q, k, r, deg, mm=inf, mem=0, outs=out: _c_call(L, fn, h, 3, n, q, k, r, deg, outs, None, mm, mem)  # noqa: E731
        assert call(40, None, 8, 2.0, 2) == 0
        assert call(40, pos, 8, 2.0, 1) == 0
        assert call(40, None, 0, 2.0, 2) == 1 and call(40, None, 33, 2.0, 2) == 1
        assert call(40, None, 8, 0.0, 2) == 1 and call(40, None, 8, -1.0, 2) == 1
        assert call(40, None, 8, inf, 2) == 1 and call(40, None, 8, nan, 2) == 1
        assert call(40, None, 8, 2.0, 0) == 1 and call(40, None, 8, 2.0, 3) == 1
        assert call(40, None, 8, 2.0, 2, -0.5) == 1 and call(40, None, 8, 2.0, 2, nan) == 1
        assert call(40, None, 8, 2.0, 2, 0.0) == 0
        assert call(40, None, 8, 2.0, 2, inf, 5) == 1
        assert call(-1, pos, 8, 2.0, 2) == 1
        assert call(1 << 31, pos, 8, 2.0, 2) == 5
        assert call(0, pos, 8, 2.0, 2) == 0
    assert _c_call(L, L.fi_points_mls_project, None, 3, 40, None, 8, 2.0, 2, out) == 1
    line = fi.PointIndex(pos[:, 0].copy(), ndim=1)
    assert _c_call(L, L.fi_points_mls_project, line._h, 1, 40, None, 8, 2.0, 2, [np.empty(40, np.float32), None, None, None]) == 1
    for bad in (dict(k=40, radius=1.0), dict(degree=3, radius=1.0), dict()):
        with pytest.raises(ValueError):
            pi.smooth(**bad)
    with pytest.raises(ValueError):
        pi.smooth(radius=1.0, normals=np.zeros((39, 3), np.float32))
    s = fi.LatticeField([12, 10, 16], dtype="f32", rank=1, nranks=2)     # a slab context
    s.add_field_constraints(fi.Weights())
    s.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, np.array([[3.0, 4.0, 9.0]], np.float32))
    with pytest.raises(fi.FiError) as e:
        s.project(pos, radius=2.0)
    assert e.value.code == 5
