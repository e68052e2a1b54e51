"""Point-cloud cleaning on the device (fi_cloud.hip through the fi_* and fi_points_* entries and fi_cloud_thin) against the
numpy restatement of the contract (tests/cloud_reference.py): floats as bit patterns, integers and masks array-equal, the
stats struct field by field as bits.  1-, 2- and 3-D, the clouds of test_gpu_knn.py, every k at which the list's class
changes, the sizes at which a leaf, a block of the fixed-order sum or a run of a cell ends, radii that lie exactly on pair
distances, non-finite points and queries, both entry families, the error codes, clean_points against the same steps by hand,
and device tensors through a child process."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import cloud_reference as CR
from test_gpu_knn import CLOUDS, _cloud, _field, _queries

pytestmark = pytest.mark.gpu

KS = [1, 7, 8, 9, 16, 17, 32]        # the list holds 8, 16 or 32 pairs: both sides of every class edge
SIZES = [[50], [40, 30], [20, 18, 16]]
BIG = 2 ** 31 - 1


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _same_f32(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~np.isnan(want))
    assert bad.size == 0, (what, bad[:5], got[tuple(bad[:5].T)], want[tuple(bad[:5].T)])


def _same_int(got, want, dtype, what=""):
    got = np.asarray(got)
    assert got.dtype == dtype and np.array_equal(got, want), (what, np.argwhere(got != want)[:5])


def _same_stats(got, want):
    assert got["counted"] == want["counted"] and got["kept"] == want["kept"], (got, want)
    for key in ("mean", "stddev", "threshold"):
        assert np.float64(got[key]).tobytes() == np.float64(want[key]).tobytes(), (key, got, want)


def _both(fi, sizes, pos):
    D = len(sizes)
    return _field(fi, sizes, pos), fi.PointIndex(pos.reshape(-1, D), ndim=D)


def _check_neighbours(index, pos, D, ks, max_distance=math.inf, table=None):
    table = table if table is not None else CR.neighbour_table(pos, D)
    for k in ks:
        want = CR.neighbour_distances(pos, D, k, max_distance, table)
        got = index.neighbour_distances(k, max_distance)
        _same_f32(got[0], want[0], ("mean", k))
        _same_f32(got[1], want[1], ("kth", k))
        _same_int(got[2], want[2], np.int32, ("counts", k))
    return table


def _check_statistical(index, pos, D, k, ratios, max_distance=math.inf, table=None):
    mean = CR.neighbour_distances(pos, D, k, max_distance, table)[0]
    for ratio in ratios:
        wkeep, wstats = CR.statistics(mean, ratio)
        keep, stats = index.statistical_outliers(k, ratio, max_distance)
        _same_int(keep, wkeep.astype(bool), np.bool_, ("keep", k, ratio))
        _same_stats(stats, wstats)
    return wstats


def _check_radius_outliers(index, pos, D, radius, least):
    want = CR.radius_outliers(pos, D, radius, least).astype(bool)
    keep, kept = index.radius_outliers(radius, least)
    _same_int(keep, want, np.bool_, ("radius", radius, least))
    assert kept == int(want.sum())


def _check_counts(index, pos, q, D, radius, limit=BIG):
    _same_int(index.radius_count(q, radius, limit), CR.radius_count(pos, q, D, radius, limit), np.int32, ("count", radius, limit))


@pytest.mark.parametrize("kind", CLOUDS)
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "%dD" % len(s))
def test_matches_the_restatement(fi, sizes, kind):
    D = len(sizes)
    rng = np.random.default_rng(D * 37 + CLOUDS.index(kind))
    pos = _cloud(rng, kind, sizes, n=1200)
    q = np.concatenate([_queries(rng, sizes, 500), pos[:100]])
    table = CR.neighbour_table(pos, D)
    # a radius with a handful of points inside: the median distance to the 8th neighbour (0 among identical points)
    r8 = float(np.median(table[1][:, min(7, table[1].shape[1] - 1)])) if table[1].size else 1.0
    for index in _both(fi, sizes, pos):
        _check_neighbours(index, pos, D, KS, table=table)
        _check_statistical(index, pos, D, 8, [0.0, 1.0, 2.5], table=table)
        for radius, least in ((r8, 1), (r8, 8), (2 * r8, 40)):
            _check_radius_outliers(index, pos, D, radius, least)
        for radius, limit in ((0.0, BIG), (r8, BIG), (3 * r8, BIG), (3 * r8, 1), (3 * r8, 7), (math.inf, BIG), (math.inf, 100)):
            _check_counts(index, pos, q, D, radius, limit)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 3 * 256 + 5])
def test_leaf_and_block_edges(fi, n):
    """a leaf of the tree holds 16 points, a block of the fixed-order sum 256"""
    sizes = [20, 18, 16]
    rng = np.random.default_rng(n)
    pos = _queries(rng, sizes, n, 0.0)
    index = fi.PointIndex(pos)
    table = _check_neighbours(index, pos, 3, [1, 8, 16, 32])          # k >= n where n is small
    _check_statistical(index, pos, 3, 8, [1.0], table=table)
    _check_radius_outliers(index, pos, 3, 4.0, 2)
    _check_counts(index, pos, np.concatenate([pos, _queries(rng, sizes, 50)]), 3, 4.0)


@pytest.mark.parametrize("n", [64 * 256, 64 * 256 + 1])
def test_more_blocks_than_one_load_of_the_ordered_sum(fi, n):
    """64 blocks of the fixed-order sum, one load of the wave that adds them, and a 65th.  The restatement's table of all pairs
    is too slow here; the means come from neighbour_distances, which the other tests hold to it"""
    rng = np.random.default_rng(n)
    pos = rng.uniform(0.0, 1000.0, size=(n, 1)).astype(np.float32)
    index = fi.PointIndex(pos, ndim=1)
    mean = index.neighbour_distances(4)[0]
    wkeep, wstats = CR.statistics(mean, 1.0)
    keep, stats = index.statistical_outliers(4, 1.0)
    _same_int(keep, wkeep.astype(bool), np.bool_)
    _same_stats(stats, wstats)
    assert stats["counted"] == n


def test_more_neighbours_asked_than_points_exist(fi):
    sizes = [20, 18, 16]
    rng = np.random.default_rng(6)
    pos = _queries(rng, sizes, 5, 0.0)
    for index in _both(fi, sizes, pos):
        _check_neighbours(index, pos, 3, [3, 4, 5, 32])
        mean, kth, counts = index.neighbour_distances(32)
        assert np.all(counts == 4) and np.all(np.isfinite(mean))
        _check_statistical(index, pos, 3, 5, [1.0])


@pytest.mark.parametrize("D", [1, 2, 3])
def test_radii_that_lie_on_pair_distances(fi, D):
    """an integer grid: many pairs at exactly 1 and sqrt(2); the radius itself counts, the float below it does not"""
    rng = np.random.default_rng(20 + D)
    sizes = SIZES[D - 1]
    pos = rng.integers(0, 8, size=(900, D)).astype(np.float32)
    q = np.concatenate([pos[:300], rng.integers(-1, 9, size=(300, D)).astype(np.float32)])
    one, root2 = np.float32(1.0), np.sqrt(np.float32(2.0))
    for index in _both(fi, sizes, pos):
        for radius in (one, np.nextafter(one, np.float32(0)), root2, np.nextafter(root2, np.float32(0))):
            _check_counts(index, pos, q, D, float(radius))
            _check_radius_outliers(index, pos, D, float(radius), 3)
        exact = CR.radius_count(pos, q, D, 1.0)
        c = int(np.median(exact))
        assert c >= 2
        for limit in (1, c - 1, c, c + 1):
            _check_counts(index, pos, q, D, 1.0, limit)
        on, below = CR.radius_count(pos, q, D, 1.0), CR.radius_count(pos, q, D, float(np.nextafter(one, np.float32(0))))
        assert np.any(on > below)
    _check_neighbours(fi.PointIndex(pos, ndim=D), pos, D, [1, 8, 17])       # ties by ascending index, duplicates at 0


@pytest.mark.parametrize("sizes", [[64], [33, 21], [17, 13, 11]], ids=lambda s: "%dD" % len(s))
def test_non_finite_points_and_queries(fi, sizes):
    rng = np.random.default_rng(5)
    D = len(sizes)
    pos = _queries(rng, sizes, 1000, 1.0)
    pos[::7, 0] = np.nan
    pos[3::11, D - 1] = np.inf
    pos[5::13, 0] = -np.inf
    q = _queries(rng, sizes, 600)
    q[::9, 0] = np.nan
    q[4::10, D - 1] = -np.inf
    q[2] = pos[0]                                            # (a NaN point's own coordinates)
    for index in _both(fi, sizes, pos):
        table = _check_neighbours(index, pos, D, [1, 8, 12, 32])
        _check_statistical(index, pos, D, 8, [1.0], table=table)
        _check_radius_outliers(index, pos, D, 2.0, 2)
        _check_counts(index, pos, q, D, 2.5)
        _check_counts(index, pos, q, D, 2.5, 2)
    allbad = np.full((10, D), np.nan, np.float32)            # no finite point at all
    for index in _both(fi, sizes, allbad):
        mean, kth, counts = index.neighbour_distances(4)
        assert np.all(np.isnan(mean)) and np.all(np.isnan(kth)) and np.all(counts == 0)
        keep, stats = index.statistical_outliers(4, 1.0)
        assert not keep.any() and stats == {"counted": 0, "kept": 0, "mean": 0.0, "stddev": 0.0, "threshold": 0.0}
        keep, kept = index.radius_outliers(1.0, 1)
        assert not keep.any() and kept == 0
        assert list(index.radius_count(q[:20], 5.0)) == list(CR.radius_count(allbad, q[:20], D, 5.0))


@pytest.mark.parametrize("max_distance", [0.0, 0.4, 3.0])
def test_max_distance_leaves_points_without_neighbours(fi, max_distance):
    rng = np.random.default_rng(31)
    sizes = [16, 16, 16]
    pos = np.concatenate([rng.integers(0, 6, size=(500, 3)).astype(np.float32),       # duplicates: neighbours at 0
                          (20 + 7 * np.arange(40)[:, None] + rng.uniform(0, 0.3, (40, 3))).astype(np.float32)])
    for index in _both(fi, sizes, pos):
        table = _check_neighbours(index, pos, 3, [1, 5, 16, 32], max_distance)
        stats = _check_statistical(index, pos, 3, 5, [0.5, 2.0], max_distance, table)
        assert 0 < stats["counted"] < len(pos)               # the far points have m = 0: +inf, not counted, not kept
    m = CR.neighbour_distances(pos, 3, 5, max_distance, table)[2]
    assert np.any(m == 0) and np.any(m > 0)


def test_batches_prior_and_rebuilds(fi):
    sizes = [24, 20, 18]
    rng = np.random.default_rng(9)
    a, b, c = (_queries(rng, sizes, n, 1.0) for n in (700, 300, 150))
    q = _queries(rng, sizes, 400)
    f = _field(fi, sizes, a, b)
    ab = np.concatenate([a, b])
    f.add_border_prior(0.5)                                  # lattice points, not data: no part of the set
    _check_neighbours(f, ab, 3, [8, 16])
    _check_statistical(f, ab, 3, 8, [1.5])
    _check_radius_outliers(f, ab, 3, 2.0, 3)
    _check_counts(f, ab, q, 3, 3.0)
    f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, c)   # a rebuild
    abc = np.concatenate([a, b, c])
    _check_neighbours(f, abc, 3, [8])
    _check_counts(f, abc, q, 3, 3.0)
    f.clear_points()
    assert len(f.neighbour_distances(3)[0]) == 0 and np.all(f.radius_count(q, 3.0) == 0)
    keep, stats = f.statistical_outliers(3, 1.0)
    assert len(keep) == 0 and stats["counted"] == 0


def test_repeated_calls_return_the_same_bytes(fi):
    rng = np.random.default_rng(44)
    pos = _queries(rng, [20, 18, 16], 3000, 0.0)
    index = fi.PointIndex(pos)
    first = index.statistical_outliers(16, 1.0)
    for _ in range(3):
        again = index.statistical_outliers(16, 1.0)
        assert np.array_equal(first[0], again[0])
        _same_stats(again[1], first[1])


# ---- thinning ------------------------------------------------------------------------------------------------------------

def _check_thin(fi, pos, cell, origin=None, normals=None, values=None):
    D = 1 if pos.ndim == 1 else pos.shape[1]
    for mode in ("mean", "first"):
        want = CR.thin(pos, D, cell, origin, mode, normals, values)
        got = fi.thin_points(pos, cell, normals, values, origin, mode, counts=True, indices=True, cell_map=True)
        got = iter(got)
        _same_f32(next(got), want["positions"].reshape(-1, *pos.shape[1:]), ("positions", mode))
        if normals is not None:
            _same_f32(next(got), want["normals"].reshape(-1, *pos.shape[1:]), ("normals", mode))
        if values is not None:
            _same_f32(next(got), want["values"], ("values", mode))
        _same_int(next(got), want["counts"], np.int32, ("counts", mode))
        _same_int(next(got), want["indices"], np.int64, ("indices", mode))
        _same_int(next(got), want["cell_map"], np.int32, ("cell_map", mode))
    only = fi.thin_points(pos, cell, origin=origin)
    _same_f32(only, CR.thin(pos, D, cell, origin)["positions"].reshape(-1, *pos.shape[1:]))
    return want


def _attributes(rng, pos):
    nrm = rng.normal(size=(len(pos), pos.shape[1] if pos.ndim == 2 else 1)).astype(np.float32).reshape(pos.shape)
    return nrm, rng.normal(size=len(pos)).astype(np.float32)


@pytest.mark.parametrize("D", [1, 2, 3])
def test_thinning_matches_the_restatement(fi, D):
    rng = np.random.default_rng(50 + D)
    pos = rng.uniform(-9, 9, size=(3000, D)).astype(np.float32)         # negative coordinates: floorf, not truncation
    pos[::97, 0] = np.nan
    pos[5::101, D - 1] = np.inf
    nrm, val = _attributes(rng, pos)
    origin = [0.3, -1.7, 2.2][:D]
    for cell in (0.75, 2.0):
        for o in (None, origin):
            _check_thin(fi, pos, cell, o)
            w = _check_thin(fi, pos, cell, o, nrm, val)
    assert w["counts"].sum() == np.all(np.isfinite(pos), axis=1).sum() and np.any(w["cell_map"] < 0)
    _check_thin(fi, pos, 1.0, None, nrm, None)
    _check_thin(fi, pos, 1.0, None, None, val)
    if D == 1:
        _check_thin(fi, pos[:, 0].copy(), 0.5, [0.25])                   # (n,) in, (m,) out


def test_thinning_runs_that_cross_a_block_and_a_cell_that_swallows_everything(fi):
    rng = np.random.default_rng(61)
    # cells of 1: 200 cells with a point or two, then one cell with 300 members whose run of sorted slots crosses 256-borders
    sparse = rng.uniform(0, 15, size=(250, 3)).astype(np.float32)
    dense = (np.float32([20.0, 3.0, 7.0]) + rng.uniform(0, 1, size=(300, 3))).astype(np.float32)
    pos = np.concatenate([sparse, dense])[rng.permutation(550)]
    nrm, val = _attributes(rng, pos)
    w = _check_thin(fi, pos, 1.0, None, nrm, val)
    assert w["counts"].max() == 300
    w = _check_thin(fi, pos, 1000.0, [-500.0, -500.0, -500.0], nrm, val)   # one cell holds the whole cloud: slow and correct
    assert list(w["counts"]) == [550]
    opposed = np.concatenate([nrm[:275], -nrm[:275]])                      # sums that cancel: zero normals
    _check_thin(fi, pos, 1000.0, [-500.0, -500.0, -500.0], opposed, None)
    one = _check_thin(fi, pos, 1e-3)                                       # a cell a point
    assert np.all(one["counts"] == 1)


def test_thinning_empty_and_refused_inputs(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    assert fi.thin_points(np.zeros((0, 3), np.float32), 1.0).shape == (0, 3)
    got = fi.thin_points(np.full((7, 2), np.nan, np.float32), 1.0, cell_map=True)
    assert got[0].shape == (0, 2) and list(got[1]) == [-1] * 7
    p = np.array([[0.5, 0.5, 0.5], [3.0, 1.0, 1.0]], np.float32)
    out = np.empty((2, 3), np.float32)
    num = C.c_long(-1)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def call(ndim=3, n=2, pos=ptr(p), nrm=None, val=None, cell=1.0, mode=0, opos=ptr(out), onrm=None, oval=None, num=C.byref(num), mem=0):
        return L.fi_cloud_thin(ndim, n, pos, nrm, val, cell, None, mode, opos, onrm, oval, None, None, None, num, mem)
    assert call() == 0 and num.value == 2
    assert call(ndim=0) == 1 and call(ndim=4) == 1 and call(n=-1) == 1 and call(pos=None) == 1 and call(opos=None) == 1
    assert call(cell=0.0) == 1 and call(cell=-1.0) == 1 and call(cell=math.nan) == 1
    assert call(mode=2) == 1 and call(mode=-1) == 1 and call(mem=7) == 1 and call(num=None) == 1
    assert call(onrm=ptr(out)) == 1 and call(oval=ptr(out)) == 1          # outputs without the inputs they come from
    assert call(n=1 << 31) == 5
    assert call(cell=1e-6) == 1                                            # 3.0 / 1e-6 cells from the origin: |c| >= 2^20
    far = np.array([[3e38, 0.0, 0.0], [-3e38, 0.0, 0.0]], np.float32)     # p - o overflows: refused, not wrapped
    o = (C.c_float * 3)(-3e38, 0.0, 0.0)
    assert L.fi_cloud_thin(3, 2, ptr(far), None, None, 1e30, o, 0, ptr(out), None, None, None, None, None, C.byref(num), 0) == 1
    with pytest.raises(ValueError):
        fi.thin_points(p, 1.0, mode="median")
    with pytest.raises(ValueError):
        fi.thin_points(p, 1.0, normals=p[:1])


# ---- the pipeline, the error codes, device tensors ---------------------------------------------------------------------------

def test_clean_points_equals_the_steps_by_hand(fi):
    pos, stray = CR.planted_cloud(2, n=1500, planted=20)
    rng = np.random.default_rng(70)
    nrm, val = _attributes(rng, pos)
    args = dict(cell=0.5, radius=1.5, min_neighbours=2, k=8, std_ratio=1.0)
    got = fi.clean_points(pos, nrm, val, **args)
    # by hand, on the device
    p, n, v = fi.thin_points(pos, 0.5, nrm, val)
    keep, kept = fi.PointIndex(p).radius_outliers(1.5, 2)
    assert kept == keep.sum()
    p, n, v = p[keep], n[keep], v[keep]
    keep2, stats = fi.PointIndex(p).statistical_outliers(8, 1.0)
    for g, w in zip(got[:3], (p[keep2], n[keep2], v[keep2])):
        _same_f32(g, w)
    # and the restatement of the same sequence
    want = CR.clean(pos, 3, nrm, val, **args)
    for g, w in zip(got[:3], want[:3]):
        _same_f32(g, w)
    report, wreport = got[3], want[3]
    _same_stats(report.pop("stats"), wreport.pop("stats"))
    assert report == wreport and report["input"] == 1520 and report["thinned"] > 0 and report["radius"] > 0
    assert set(fi.clean_points(pos, k=8)[3]) == {"input", "statistical", "stats", "output"}
    only = fi.clean_points(pos, radius=1.5)
    assert only[1] is None and only[2] is None and only[3]["radius"] == 20 and np.array_equal(only[0], pos[~stray])


def test_device_tensors(tmp_path):
    """torch device tensors in, torch device tensors out, equal to the restatement; in a fresh process
    (tests/cloud_torch_worker.py), as torch must stay out of this one"""
    pos, _ = CR.planted_cloud(3, n=1500, planted=12)
    rng = np.random.default_rng(71)
    nrm, val = _attributes(rng, pos)
    q = _queries(rng, [32, 32, 32], 500)
    np.savez(tmp_path / "in.npz", pos=pos, nrm=nrm, val=val, q=q)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cloud_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"].all()
    for ours in ("pts", "ctx"):
        _same_int(o[ours + "_count"], CR.radius_count(pos, q, 3, 1.5, 6), np.int32)
        mean, kth, counts = CR.neighbour_distances(pos, 3, 12)
        _same_f32(o[ours + "_mean"], mean)
        _same_f32(o[ours + "_kth"], kth)
        _same_int(o[ours + "_m"], counts, np.int32)
        wkeep, wstats = CR.statistics(mean, 1.0)
        _same_int(o[ours + "_stat_keep"], wkeep.astype(bool), np.bool_)
        assert np.array_equal(o[ours + "_stats"].view(np.uint64),
                              np.array([wstats["counted"], wstats["kept"], wstats["mean"], wstats["stddev"], wstats["threshold"]]).view(np.uint64))
        _same_int(o[ours + "_radius_keep"], CR.radius_outliers(pos, 3, 1.5, 2).astype(bool), np.bool_)
    t = CR.thin(pos, 3, 0.75, [0.1, 0.2, 0.3], CR.MEAN, nrm, val)
    for key in ("positions", "normals", "values"):
        _same_f32(o["thin_" + key], t[key])
    _same_int(o["thin_counts"], t["counts"], np.int32)
    _same_int(o["thin_indices"], t["indices"], np.int64)
    _same_int(o["thin_cell_map"], t["cell_map"], np.int32)
    want = CR.clean(pos, 3, nrm, val, cell=0.5, radius=1.5, k=8, std_ratio=1.0)
    for key, w in zip(("clean_pos", "clean_nrm", "clean_val"), want[:3]):
        _same_f32(o[key], w)


def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    f = _field(fi, [10, 10, 10], np.ones((4, 3), np.float32))
    q = np.ones((4, 3), np.float32)
    c = np.empty(4, np.int32)
    m = np.empty(4, np.float32)
    keep = np.empty(4, np.uint8)
    stats = _capi.FiOutlierStats()
    kept = C.c_long(0)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    h = C.c_void_p()
    assert L.fi_points_create(C.byref(h), 3, 4, ptr(q), 0) == 0
    try:
        for count, handle in ((L.fi_radius_count, f._h), (L.fi_points_radius_count, h)):
            assert count(handle, 4, ptr(q), 1.0, 1, ptr(c), 0) == 0
            assert count(handle, 4, ptr(q), math.inf, BIG, ptr(c), 0) == 0 and list(c) == [4] * 4
            assert count(handle, 4, ptr(q), math.nan, 1, ptr(c), 0) == 1
            assert count(handle, 4, ptr(q), -1.0, 1, ptr(c), 0) == 1
            assert count(handle, 4, ptr(q), 1.0, 0, ptr(c), 0) == 1
            assert count(handle, -1, ptr(q), 1.0, 1, ptr(c), 0) == 1
            assert count(handle, 4, None, 1.0, 1, ptr(c), 0) == 1
            assert count(handle, 4, ptr(q), 1.0, 1, None, 0) == 1
            assert count(handle, 4, ptr(q), 1.0, 1, ptr(c), 7) == 1
            assert count(handle, 1 << 31, ptr(q), 1.0, 1, ptr(c), 0) == 5
        for dist, handle in ((L.fi_neighbour_distances, f._h), (L.fi_points_neighbour_distances, h)):
            assert dist(handle, 3, math.inf, ptr(m), None, None, 0) == 0
            assert dist(handle, 3, math.inf, None, ptr(m), None, 0) == 0
            assert dist(handle, 3, math.inf, None, None, ptr(c), 0) == 0 and list(c) == [3] * 4
            assert dist(handle, 3, math.inf, None, None, None, 0) == 1
            assert dist(handle, 0, math.inf, ptr(m), None, None, 0) == 1
            assert dist(handle, 33, math.inf, ptr(m), None, None, 0) == 1
            assert dist(handle, 3, math.nan, ptr(m), None, None, 0) == 1
            assert dist(handle, 3, -1.0, ptr(m), None, None, 0) == 1
            assert dist(handle, 3, math.inf, ptr(m), None, None, 7) == 1
        for stat, handle in ((L.fi_outliers_statistical, f._h), (L.fi_points_outliers_statistical, h)):
            assert stat(handle, 3, math.inf, 1.0, ptr(keep), C.byref(stats), 0) == 0 and stats.counted == 4
            assert stat(handle, 3, math.inf, 1.0, None, C.byref(stats), 0) == 0
            assert stat(handle, 3, math.inf, 1.0, ptr(keep), None, 0) == 0
            assert stat(handle, 3, math.inf, 1.0, None, None, 0) == 1
            assert stat(handle, 3, math.inf, math.nan, ptr(keep), None, 0) == 1
            assert stat(handle, 3, math.inf, -0.5, ptr(keep), None, 0) == 1
            assert stat(handle, 40, math.inf, 1.0, ptr(keep), None, 0) == 1
            assert stat(handle, 3, -1.0, 1.0, ptr(keep), None, 0) == 1
            assert stat(handle, 3, math.inf, 1.0, ptr(keep), None, 9) == 1
        for rad, handle in ((L.fi_outliers_radius, f._h), (L.fi_points_outliers_radius, h)):
            assert rad(handle, 1.0, 2, ptr(keep), C.byref(kept), 0) == 0 and kept.value == 4 and list(keep) == [1] * 4
            assert rad(handle, 1.0, 2, None, C.byref(kept), 0) == 0 and rad(handle, 1.0, 2, ptr(keep), None, 0) == 0
            assert rad(handle, 1.0, 2, None, None, 0) == 1
            assert rad(handle, 1.0, 0, ptr(keep), None, 0) == 1
            assert rad(handle, math.nan, 2, ptr(keep), None, 0) == 1
            assert rad(handle, -2.0, 2, ptr(keep), None, 0) == 1
            assert rad(handle, 1.0, 2, ptr(keep), None, 5) == 1
        assert L.fi_points_radius_count(None, 4, ptr(q), 1.0, 1, ptr(c), 0) == 1
        assert L.fi_points_neighbour_distances(None, 3, math.inf, ptr(m), None, None, 0) == 1
        assert L.fi_points_outliers_statistical(None, 3, math.inf, 1.0, ptr(keep), None, 0) == 1
        assert L.fi_points_outliers_radius(None, 1.0, 2, ptr(keep), None, 0) == 1
    finally:
        L.fi_points_destroy(h)
    with pytest.raises(ValueError):
        f.neighbour_distances(40)
    s = fi.LatticeField([12, 10, 16], dtype="f32", rank=1, nranks=2)     # a slab context
    s.add_field_constraints(fi.Weights())
    s.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, np.array([[3.0, 4.0, 9.0]], np.float32))
    for refused in (lambda: s.radius_count(q, 1.0), lambda: s.neighbour_distances(3), lambda: s.statistical_outliers(3),
                    lambda: s.radius_outliers(1.0)):
        with pytest.raises(fi.FiError) as e:
            refused()
        assert e.value.code == 5
