"""Nearest data points on the device (fi_nearest.hip through fi_nearest, fi_distance_field and fi_points_*) against the numpy
oracle of the contract (tests/nearest_reference.py), distances and indices array-equal: 1-, 2- and 3-D, degenerate clouds,
far queries, non-finite points and queries, max_distance, empty sets, host and device buffers, several batches with the
border prior's left out, rebuilds, the distance field, the context-free PointIndex and the error codes.  Then the border
prior: its rows and its solved field equal with and without FI_BORDER_BRUTE (the reference's brute force)."""
import ctypes as C
import math

import numpy as np
import pytest

import nearest_reference as R
from util import sphere_points

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _same(got, want):
    gd, gi = got
    wd, wi = want
    gd, gi = np.asarray(gd), np.asarray(gi)
    assert gd.dtype == np.float32 and gi.dtype == np.int64
    assert np.array_equal(np.isnan(gd), np.isnan(wd))
    bad = np.flatnonzero((gd.view(np.uint32) != wd.view(np.uint32)) & ~np.isnan(wd))
    assert bad.size == 0, (bad[:5], gd[bad[:5]], wd[bad[:5]], gi[bad[:5]], wi[bad[:5]])
    assert np.array_equal(gi, wi), np.flatnonzero(gi != wi)[:5]


def _field(fi, sizes, *batches):
    f = fi.LatticeField(sizes)
    f.add_field_constraints(fi.Weights())
    for p in batches:
        f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, p)
    return f


def _queries(rng, sizes, n, pad=5.0):
    D = len(sizes)
    return np.stack([rng.uniform(-pad, s - 1 + pad, n) for s in sizes], 1).astype(np.float32).reshape(n, D)


def _check(fi, sizes, pos, q, max_distance=math.inf):
    D = len(sizes)
    want = R.nearest(pos, q, D, max_distance)
    f = _field(fi, sizes, pos)
    _same(f.nearest(q, max_distance=max_distance, indices=True), want)
    _same(fi.PointIndex(pos.reshape(-1, D), ndim=D).nearest(q, max_distance=max_distance, indices=True), want)
    return f


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
    q = np.concatenate([_queries(rng, sizes, 3000), R.lattice_points(sizes)[:500], pos[:200]])
    if kind == "cluster":                                    # queries 10^3 lattice units away
        q = np.concatenate([q, (np.float32(2.0) + rng.normal(size=(500, len(sizes))) * 1000).astype(np.float32)])
    _check(fi, sizes, pos, q)


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
    _check(fi, sizes, pos, q)
    allbad = np.full((10, D), np.nan, np.float32)            # no finite point: +inf / -1
    _check(fi, sizes, allbad, q)


@pytest.mark.parametrize("max_distance", [0.0, 0.5, 3.0, math.inf])
@pytest.mark.parametrize("sizes", [[80], [30, 30], [16, 16, 16]], ids=lambda s: "%dD" % len(s))
def test_max_distance(fi, sizes, max_distance):
    rng = np.random.default_rng(len(sizes) * 7 + [0.0, 0.5, 3.0, math.inf].index(max_distance))
    pos = rng.integers(0, 12, size=(300, len(sizes))).astype(np.float32)
    q = np.concatenate([_queries(rng, sizes, 2000), R.lattice_points(sizes)])
    f = _check(fi, sizes, pos, q, max_distance)
    _same(f.distance_field(max_distance=max_distance, indices=True), R.distance_field(pos, sizes, max_distance))


def test_empty_sets_and_queries(fi):
    sizes = [12, 10, 8]
    q = np.ones((5, 3), np.float32)
    pi = fi.PointIndex(np.zeros((0, 3), np.float32))
    d, i = pi.nearest(q, indices=True)
    assert np.all(np.isinf(d)) and np.all(i == -1)
    d, i = pi.distance_field(sizes, indices=True)
    assert d.shape == (960,) and np.all(np.isinf(d)) and np.all(i == -1)
    f = _field(fi, sizes)                                    # a context without points
    d, i = f.nearest(q, indices=True)
    assert np.all(np.isinf(d)) and np.all(i == -1)
    f = _field(fi, sizes, q)
    d, i = f.nearest(np.zeros((0, 3), np.float32), indices=True)
    assert d.shape == (0,) and i.shape == (0,)
    assert f.nearest(np.zeros((0, 3), np.float32)).shape == (0,)


def test_device_tensors(tmp_path):
    """torch device tensors in, torch device tensors out (int64 indices), equal to the oracle; in a fresh process
    (tests/nearest_torch_worker.py), as torch must stay out of this one"""
    import os
    import subprocess
    import sys
    sizes = [30, 26, 22]
    rng = np.random.default_rng(8)
    pos, _ = sphere_points(rng, sizes, 5000)
    q = _queries(rng, sizes, 4000)
    np.savez(tmp_path / "in.npz", sizes=np.array(sizes), pos=pos, q=q)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nearest_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"][0] and o["field_on_device"][0] and o["empty_ok"][0]
    want = R.nearest(pos, q, 3)
    _same((o["ctx_d"], o["ctx_i"]), want)
    _same((o["pts_d"], o["pts_i"]), want)
    assert np.array_equal(o["ctx_d_only"].view(np.uint32), want[0].view(np.uint32))
    wf = R.distance_field(pos, sizes)
    _same((o["ctx_fd"], o["ctx_fi"]), wf)
    _same((o["pts_fd"], o["pts_fi"]), wf)


def test_batches_prior_and_rebuilds(fi):
    sizes = [24, 20, 18]
    rng = np.random.default_rng(9)
    a = _queries(rng, sizes, 1500, 1.0)
    b = _queries(rng, sizes, 700, 1.0)
    c = _queries(rng, sizes, 300, 1.0)
    q = np.concatenate([_queries(rng, sizes, 2000), R.lattice_points(sizes)[::3]])
    f = _field(fi, sizes, a, b)
    _same(f.nearest(q, indices=True), R.nearest(np.concatenate([a, b]), q, 3))
    f.add_border_prior(0.5)                                  # lattice points, not data: no index of the set
    _same(f.nearest(q, indices=True), R.nearest(np.concatenate([a, b]), q, 3))
    f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, c)   # a rebuild
    _same(f.nearest(q, indices=True), R.nearest(np.concatenate([a, b, c]), q, 3))
    _same(f.distance_field(indices=True), R.distance_field(np.concatenate([a, b, c]), sizes))
    f.clear_points()
    d, i = f.nearest(q, indices=True)
    assert np.all(np.isinf(d)) and np.all(i == -1)
    f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, c)
    _same(f.nearest(q, indices=True), R.nearest(c, q, 3))


@pytest.mark.parametrize("sizes", [[300], [70, 50], [33, 29, 25]], ids=lambda s: "%dD" % len(s))
def test_distance_field_equals_nearest_at_the_lattice_points(fi, sizes):
    rng = np.random.default_rng(len(sizes))
    pos = _queries(rng, sizes, 3000, 3.0) if len(sizes) < 3 else sphere_points(rng, sizes, 3000)[0]
    f = _field(fi, sizes, pos)
    got = f.distance_field(indices=True)
    _same(got, R.distance_field(pos, sizes))
    _same(got, f.nearest(R.lattice_points(sizes), indices=True))
    assert np.array_equal(f.distance_field(), got[0])
    _same(fi.PointIndex(pos.reshape(-1, len(sizes)), ndim=len(sizes)).distance_field(sizes, indices=True), got)


def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    f = _field(fi, [10, 10, 10], np.ones((4, 3), np.float32))
    q = np.ones((4, 3), np.float32)
    d = np.empty(4, np.float32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert L.fi_nearest(f._h, -1, ptr(q), math.inf, ptr(d), None, 0) == 1
    assert L.fi_nearest(f._h, 4, None, math.inf, ptr(d), None, 0) == 1
    assert L.fi_nearest(f._h, 4, ptr(q), math.inf, None, None, 0) == 1
    assert L.fi_nearest(f._h, 4, ptr(q), math.nan, ptr(d), None, 0) == 1
    assert L.fi_nearest(f._h, 4, ptr(q), -1.0, ptr(d), None, 0) == 1
    assert L.fi_nearest(f._h, 4, ptr(q), math.inf, ptr(d), None, 7) == 1
    assert L.fi_nearest(f._h, 1 << 31, ptr(q), math.inf, ptr(d), None, 0) == 5
    assert L.fi_distance_field(f._h, math.inf, None, None, 0) == 1
    assert L.fi_distance_field(f._h, -0.5, ptr(d), None, 0) == 1
    h = C.c_void_p()
    assert L.fi_points_create(C.byref(h), 0, 4, ptr(q), 0) == 1
    assert L.fi_points_create(C.byref(h), 4, 4, ptr(q), 0) == 1
    assert L.fi_points_create(C.byref(h), 3, -1, ptr(q), 0) == 1
    assert L.fi_points_create(C.byref(h), 3, 4, None, 0) == 1
    assert L.fi_points_create(C.byref(h), 3, 4, ptr(q), 2) == 1
    assert L.fi_points_create(C.byref(h), 3, 1 << 31, ptr(q), 0) == 5
    assert L.fi_points_create(C.byref(h), 3, 4, ptr(q), 0) == 0
    try:
        assert L.fi_points_nearest(h, 4, ptr(q), math.nan, ptr(d), None, 0) == 1
        assert L.fi_points_nearest(h, 4, ptr(q), math.inf, ptr(d), None, 0) == 0
        sz = (C.c_int * 3)(4, 0, 4)
        assert L.fi_points_distance_field(h, sz, math.inf, ptr(d), None, 0) == 1
        assert L.fi_points_distance_field(h, None, math.inf, ptr(d), None, 0) == 1
    finally:
        L.fi_points_destroy(h)
    s = fi.LatticeField([12, 10, 16], dtype="f32", rank=1, nranks=2)     # a slab context
    s.add_field_constraints(fi.Weights())
    s.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, np.array([[3.0, 4.0, 9.0]], np.float32))
    with pytest.raises(fi.FiError) as e:
        s.nearest(q)
    assert e.value.code == 5
    with pytest.raises(fi.FiError) as e:
        s.distance_field()
    assert e.value.code == 5


# ---- the border prior: the tree search against the reference's brute force (FI_BORDER_BRUTE) ------------------------------

def _prior(fi, sizes, pos, nrm, monkeypatch, brute, dtype="f32"):
    if brute:
        monkeypatch.setenv("FI_BORDER_BRUTE", "1")
    else:
        monkeypatch.delenv("FI_BORDER_BRUTE", raising=False)
    try:
        w = fi.Weights()
        f = fi.LatticeField(sizes, dtype=dtype)
        f.add_field_constraints(w)
        f.add_points(w.data_pos, w.value_kernel, w.data_gradient if nrm is not None else 0.0, w.gradient_kernel, pos, nrm)
        f.add_border_prior(0.001)
        f.assemble()
    finally:
        monkeypatch.delenv("FI_BORDER_BRUTE", raising=False)
    return f


@pytest.mark.parametrize("case", ["2-D 1024^2, 10 k points", "3-D 64^3, 50 k sphere points", "3-D 256^3, 1 M points"])
def test_border_prior_rows_equal_the_brute_force(fi, case, monkeypatch):
    rng = np.random.default_rng(77)
    if case.startswith("2-D"):
        sizes = [1024, 1024]
        pos = _queries(rng, sizes, 10000, 20.0)
        nrm = None
    elif "64" in case:
        sizes = [64, 64, 64]
        pos, nrm = sphere_points(rng, sizes, 50000)
    else:
        sizes = [256, 256, 256]
        pos, nrm = sphere_points(rng, sizes, 1000000, noise=2.0)
    fs = [_prior(fi, sizes, pos, nrm, monkeypatch, brute) for brute in (False, True)]
    assert np.array_equal(fs[0].Atb(), fs[1].Atb())
    assert np.array_equal(fs[0].diag(), fs[1].diag())
    x = rng.normal(size=int(np.prod(sizes)))
    assert np.array_equal(fs[0].apply_AtA(x), fs[1].apply_AtA(x))


def test_border_prior_solved_field_equals_the_brute_force(fi, monkeypatch):
    """sdf_from_points, the prior at the reference's default weight, a solve: the same field bit for bit"""
    sizes = [48, 40, 44]
    pos, nrm = sphere_points(np.random.default_rng(12), sizes, 8000)
    out = []
    for brute in (False, True):
        f = fi.sdf_from_points(sizes, fi.Weights(), pos, nrm)
        if brute:
            monkeypatch.setenv("FI_BORDER_BRUTE", "1")
        f.add_border_prior(0.001)
        monkeypatch.delenv("FI_BORDER_BRUTE", raising=False)
        out.append(fi.solve_sparse_linear_with_guess(f, np.zeros(f.num_unknowns, np.float32), 200, 1e-5))
    assert out[0] is not None and np.array_equal(out[0], out[1])
