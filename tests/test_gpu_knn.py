"""Exact k nearest data points on the device (fi_knn.hip through fi_knn and fi_points_knn) against the numpy oracle of the
contract (tests/normals_reference.py knn): distances as bit patterns, indices array-equal.  1-, 2- and 3-D, degenerate
clouds, every k at which the kernel class changes, k = 1 against nearest(), more neighbours asked than points exist,
non-finite points and queries, max_distance, several batches with the border prior's left out, rebuilds, host and device
buffers and the error codes."""
import ctypes as C
import math

import numpy as np
import pytest

import nearest_reference as NR
import normals_reference as R
from util import sphere_points

pytestmark = pytest.mark.gpu

KS = [1, 2, 8, 9, 16, 17, 32]        # the kernels hold 8, 16 or 32 pairs: both sides of every class edge


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _same(got, want, k):
    gd, gi = np.asarray(got[0]), np.asarray(got[1])
    wd, wi = want[0][:, :k], want[1][:, :k]                   # (a smaller k is a prefix of a larger one's result)
    assert gd.dtype == np.float32 and gi.dtype == np.int64 and gd.shape == wd.shape and gi.shape == wi.shape
    assert np.array_equal(np.isnan(gd), np.isnan(wd))
    bad = np.argwhere((gd.view(np.uint32) != wd.view(np.uint32)) & ~np.isnan(wd))
    assert bad.size == 0, (k, bad[:5], gd[bad[:5, 0]], wd[bad[:5, 0]], gi[bad[:5, 0]], wi[bad[:5, 0]])
    assert np.array_equal(gi, wi), (k, np.argwhere(gi != wi)[:5])


def _field(fi, sizes, *batches):
    f = fi.LatticeField(sizes)
    f.add_field_constraints(fi.Weights())
    for p in batches:
        f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, p)
    return f


def _queries(rng, sizes, n, pad=5.0):
    D = len(sizes)
    return np.stack([rng.uniform(-pad, s - 1 + pad, n) for s in sizes], 1).astype(np.float32).reshape(n, D)


def _check(fi, sizes, pos, q, max_distance=math.inf, ks=KS):
    D = len(sizes)
    want = R.knn(pos, q, D, max(ks), max_distance)
    f = _field(fi, sizes, pos)
    pi = fi.PointIndex(pos.reshape(-1, D), ndim=D)
    for k in ks:
        _same(f.knn(q, k, max_distance=max_distance), want, k)
        _same(pi.knn(q, k, max_distance=max_distance), want, k)
    return f, want


CLOUDS = ["random", "identical", "collinear", "cluster", "single", "outside", "grid ties"]


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
@pytest.mark.parametrize("sizes", [[50], [40, 30], [20, 18, 16]], ids=lambda s: "%dD" % len(s))
def test_matches_the_oracle(fi, sizes, kind):
    rng = np.random.default_rng(len(sizes) * 31 + CLOUDS.index(kind))
    pos = _cloud(rng, kind, sizes)
    q = np.concatenate([_queries(rng, sizes, 3000), NR.lattice_points(sizes)[:500], pos[:200]])
    if kind == "cluster":                                    # queries 10^3 lattice units away
        q = np.concatenate([q, (np.float32(2.0) + rng.normal(size=(500, len(sizes))) * 1000).astype(np.float32)])
    f, want = _check(fi, sizes, pos, q)
    # k = 1 is nearest(), bit for bit; distances alone are the same distances
    d1, i1 = f.knn(q, 1)
    nd, ni = f.nearest(q, indices=True)
    assert np.array_equal(d1[:, 0].view(np.uint32), nd.view(np.uint32)) and np.array_equal(i1[:, 0], ni)
    assert np.array_equal(f.knn(q, 9, indices=False).view(np.uint32), want[0][:, :9].view(np.uint32))


def test_a_point_finds_itself_or_an_earlier_duplicate(fi):
    rng = np.random.default_rng(4)
    pos = rng.integers(0, 6, size=(3000, 3)).astype(np.float32)
    d, i = fi.PointIndex(pos).knn(pos, 4)
    assert np.all(d[:, 0] == 0)
    first = {}
    for j, p in enumerate(map(tuple, pos)):
        first.setdefault(p, j)
    assert np.array_equal(i[:, 0], np.array([first[tuple(p)] for p in pos]))


def test_more_neighbours_asked_than_points_exist(fi):
    sizes = [20, 18, 16]
    rng = np.random.default_rng(6)
    pos = _queries(rng, sizes, 5, 0.0)
    q = _queries(rng, sizes, 300)
    _, want = _check(fi, sizes, pos, q, ks=[4, 5, 6, 32])
    assert np.all(want[1][:, :5] >= 0) and np.all(want[1][:, 5:] == -1) and np.all(np.isinf(want[0][:, 5:]))


@pytest.mark.parametrize("sizes", [[64], [33, 21], [17, 13, 11]], ids=lambda s: "%dD" % len(s))
def test_non_finite_points_and_queries(fi, sizes):
    rng = np.random.default_rng(5)
    D = len(sizes)
    pos = _queries(rng, sizes, 2000, 1.0)
    pos[::7, 0] = np.nan
    pos[3::11, D - 1] = np.inf
    pos[5::13, 0] = -np.inf
    q = _queries(rng, sizes, 1500)
    q[::9, 0] = np.nan
    q[4::10, D - 1] = -np.inf
    q[2] = pos[0]                                            # (a NaN point's own coordinates)
    _check(fi, sizes, pos, q, ks=[1, 8, 12, 32])
    allbad = np.full((10, D), np.nan, np.float32)            # no finite point: +inf / -1
    _check(fi, sizes, allbad, q, ks=[1, 20])


@pytest.mark.parametrize("max_distance", [0.0, 0.5, 3.0, math.inf])
@pytest.mark.parametrize("sizes", [[80], [30, 30], [16, 16, 16]], ids=lambda s: "%dD" % len(s))
def test_max_distance(fi, sizes, max_distance):
    rng = np.random.default_rng(len(sizes) * 7 + [0.0, 0.5, 3.0, math.inf].index(max_distance))
    pos = rng.integers(0, 12, size=(300, len(sizes))).astype(np.float32)
    q = np.concatenate([_queries(rng, sizes, 2000), NR.lattice_points(sizes)])
    _check(fi, sizes, pos, q, max_distance, ks=[1, 5, 16, 32])


def test_empty_sets_and_queries(fi):
    q = np.ones((5, 3), np.float32)
    d, i = fi.PointIndex(np.zeros((0, 3), np.float32)).knn(q, 3)
    assert d.shape == (5, 3) and np.all(np.isinf(d)) and np.all(i == -1)
    f = _field(fi, [12, 10, 8], q)
    d, i = f.knn(np.zeros((0, 3), np.float32), 7)
    assert d.shape == (0, 7) and i.shape == (0, 7)


def test_batches_prior_and_rebuilds(fi):
    sizes = [24, 20, 18]
    rng = np.random.default_rng(9)
    a = _queries(rng, sizes, 1500, 1.0)
    b = _queries(rng, sizes, 700, 1.0)
    c = _queries(rng, sizes, 300, 1.0)
    q = np.concatenate([_queries(rng, sizes, 1500), NR.lattice_points(sizes)[::5]])
    f = _field(fi, sizes, a, b)
    want = R.knn(np.concatenate([a, b]), q, 3, 12)
    _same(f.knn(q, 12), want, 12)
    f.add_border_prior(0.5)                                  # lattice points, not data: no index of the set
    _same(f.knn(q, 12), want, 12)
    f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, c)   # a rebuild
    _same(f.knn(q, 12), R.knn(np.concatenate([a, b, c]), q, 3, 12), 12)
    f.clear_points()
    d, i = f.knn(q, 3)
    assert np.all(np.isinf(d)) and np.all(i == -1)
    f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, c)
    _same(f.knn(q, 12), R.knn(c, q, 3, 12), 12)


def test_device_tensors(tmp_path):
    """torch device tensors in, torch device tensors out, equal to the host path's oracle; in a fresh process
    (tests/knn_torch_worker.py), as torch must stay out of this one"""
    import os
    import subprocess
    import sys
    sizes = [30, 26, 22]
    rng = np.random.default_rng(8)
    pos, _ = sphere_points(rng, sizes, 3000)
    q = _queries(rng, sizes, 2000)
    np.savez(tmp_path / "in.npz", sizes=np.array(sizes), pos=pos, q=q, k=np.array([12]), view=np.zeros((1, 3), np.float32))
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "knn_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"][0] and o["empty_ok"][0]
    want = R.knn(pos, q, 3, 12)
    _same((o["ctx_d"], o["ctx_i"]), want, 12)
    _same((o["pts_d"], o["pts_i"]), want, 12)
    assert np.array_equal(o["ctx_d_only"].view(np.uint32), want[0].view(np.uint32))


def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    f = _field(fi, [10, 10, 10], np.ones((4, 3), np.float32))
    q = np.ones((4, 3), np.float32)
    d = np.empty(4 * 32, np.float32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert L.fi_knn(f._h, 4, ptr(q), 3, math.inf, ptr(d), None, 0) == 0
    assert L.fi_knn(f._h, 4, ptr(q), 0, math.inf, ptr(d), None, 0) == 1
    assert L.fi_knn(f._h, 4, ptr(q), 33, math.inf, ptr(d), None, 0) == 1
    assert L.fi_knn(f._h, -1, ptr(q), 3, math.inf, ptr(d), None, 0) == 1
    assert L.fi_knn(f._h, 4, None, 3, math.inf, ptr(d), None, 0) == 1
    assert L.fi_knn(f._h, 4, ptr(q), 3, math.inf, None, None, 0) == 1
    assert L.fi_knn(f._h, 4, ptr(q), 3, math.nan, ptr(d), None, 0) == 1
    assert L.fi_knn(f._h, 4, ptr(q), 3, -1.0, ptr(d), None, 0) == 1
    assert L.fi_knn(f._h, 4, ptr(q), 3, math.inf, ptr(d), None, 7) == 1
    assert L.fi_knn(f._h, 1 << 31, ptr(q), 3, math.inf, ptr(d), None, 0) == 5
    h = C.c_void_p()
    assert L.fi_points_create(C.byref(h), 3, 4, ptr(q), 0) == 0
    try:
        assert L.fi_points_knn(None, 4, ptr(q), 3, math.inf, ptr(d), None, 0) == 1
        assert L.fi_points_knn(h, 4, ptr(q), 33, math.inf, ptr(d), None, 0) == 1
        assert L.fi_points_knn(h, 4, ptr(q), 32, math.inf, ptr(d), None, 0) == 0
    finally:
        L.fi_points_destroy(h)
    with pytest.raises(ValueError):
        f.knn(q, 40)
    s = fi.LatticeField([12, 10, 16], dtype="f32", rank=1, nranks=2)     # a slab context
    s.add_field_constraints(fi.Weights())
    s.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, np.array([[3.0, 4.0, 9.0]], np.float32))
    with pytest.raises(fi.FiError) as e:
        s.knn(q, 3)
    assert e.value.code == 5
