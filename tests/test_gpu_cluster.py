"""Point-cloud clustering on the device (fi_cluster.hip through fi_cluster, fi_points_cluster and fi_cluster_measure) against
the numpy restatement of the contract (tests/cluster_reference.py): labels, core masks and every stats field array-equal, the
rows' integers equal and their floats and doubles as bit patterns.  1-, 2- and 3-D, the clouds of test_gpu_knn.py at the
sizes where a leaf, a chunk of the centroid sum and a workgroup end, eps that lie exactly on pair distances, a chain across
twenty workgroups, duplicates, a border tie, noise only, non-finite points, both entry families, the error codes,
clean_points against the same steps by hand, and device tensors through a child process."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import cloud_reference as CR
import cluster_reference as KR
from test_gpu_knn import CLOUDS, _cloud, _field

pytestmark = pytest.mark.gpu

SIZES = [[50], [40, 30], [20, 18, 16]]
COUNTS = [15, 16, 17, 255, 256, 257, 1000]     # both sides of a leaf (16), of a chunk of the centroid sum and a workgroup (256)
LEAST = [1, 2, 4, 9]
ONE = np.float32(1.0)
EPS23 = np.float32(2.0 ** -23)                  # nextafter(1, 2) - 1


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _both(fi, sizes, pos):
    D = len(sizes)
    return _field(fi, sizes, pos), fi.PointIndex(pos.reshape(-1, D), ndim=D)


def _same_rows(got, want, D, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for c, (g, w) in enumerate(zip(got, want)):
        assert g["count"] == w["count"] and g["core"] == w["core"], (what, c, g, w)
        for key, kind in (("lo", np.uint32), ("hi", np.uint32), ("centroid", np.uint64)):
            assert g[key].dtype == w[key].dtype and g[key].shape == (D,), (what, c, key)
            assert np.array_equal(g[key].view(kind), w[key][:D].view(kind)), (what, c, key, g[key], w[key])


def _check(fi, indices, pos, D, eps, least, table=True):
    """every index against the restatement of (eps, least): labels, core, stats; the table once"""
    want = KR.cluster(pos, D, eps, least)
    for index in indices:
        labels, core, stats = index.cluster(eps, least, core=True, stats=True)
        what = (type(index).__name__, D, len(pos), eps, least)
        assert labels.dtype == np.int32 and np.array_equal(labels, want[0]), (what, np.flatnonzero(labels != want[0])[:5])
        assert core.dtype == np.bool_ and np.array_equal(core, want[1].astype(bool)), what
        assert stats == want[2], (what, stats, want[2])
        assert np.array_equal(index.cluster(eps, least), want[0]), what          # labels alone
    if table:
        shaped = pos.reshape(-1, D)
        rows = fi.cluster_measure(shaped, want[0], want[1])
        _same_rows(rows, KR.measure(shaped, D, want[0], want[1], want[2]["clusters"]), D, (D, len(pos), eps, least))
    return want


def _median_nn(pos, D):
    d = CR.neighbour_table(pos, D, 1)[1]
    return float(np.median(d[:, 0])) if d.size else 1.0


@pytest.mark.parametrize("kind", CLOUDS)
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "%dD" % len(s))
def test_matches_the_restatement(fi, sizes, kind):
    D = len(sizes)
    for n in COUNTS:
        rng = np.random.default_rng(1000 * D + 10 * CLOUDS.index(kind) + n)
        pos = _cloud(rng, kind, sizes, n=n)
        if len(pos) == 0 or (kind == "single" and n > COUNTS[0]):
            continue                                         # ("identical" is n // 4 points, "single" one point at every n)
        indices = _both(fi, sizes, pos)
        nn = _median_nn(pos, D)
        for eps in (nn, 2.0 * nn):                           # many clusters, then few
            for least in LEAST:
                _check(fi, indices, pos, D, eps, least)


@pytest.mark.parametrize("D", [1, 2, 3])
def test_eps_that_lie_on_pair_distances(fi, D):
    """an integer grid, every s exact: many pairs at exactly 1 and sqrt(2); the pair at eps joins, the float below eps does not"""
    rng = np.random.default_rng(20 + D)
    pos = rng.integers(0, 8, size=([40, 150, 600][D - 1], D)).astype(np.float32)
    root2 = np.sqrt(np.float32(2.0))
    indices = _both(fi, SIZES[D - 1], pos)
    clusters = {}
    for eps in (ONE, np.nextafter(ONE, np.float32(0)), root2, np.nextafter(root2, np.float32(0))):
        for least in (1, 4):
            clusters[float(eps), least] = _check(fi, indices, pos, D, float(eps), least)[2]["clusters"]
    assert clusters[1.0, 1] < clusters[float(np.nextafter(ONE, np.float32(0))), 1]
    if D > 1:
        assert clusters[float(root2), 1] < clusters[float(np.nextafter(root2, np.float32(0))), 1]


def _chain(D, n, stretched):
    """a polyline of n points at spacing 1 -- along x in 1-D, a staircase of unit steps along x, y, z in turn in 3-D, whose
    points other than neighbours lie sqrt(2) or more apart -- with the link behind its first points stretched to
    nextafter(1, 2) on request: those points move by -2^-23 along x, where coordinates of 0 and 1 have the bits for it"""
    k = np.arange(n)
    if D == 1:
        pos, short = k.astype(np.float32).reshape(-1, 1), 2   # the link 1 -> 2
    else:
        pos = np.stack([(k + 2) // 3, (k + 1) // 3, k // 3], 1).astype(np.float32)
        short = 4                                             # the link 3 -> 4 runs along x: (1, 1, 1) -> (2, 1, 1)
    if stretched:
        pos[:short, 0] -= EPS23
        assert pos[short, 0] - pos[short - 1, 0] == np.nextafter(ONE, np.float32(2))
    return pos, short


@pytest.mark.parametrize("stretched", [False, True], ids=["whole", "stretched"])
@pytest.mark.parametrize("D", [1, 3])
def test_a_chain_across_twenty_workgroups(fi, D, stretched):
    n = 5000
    pos, short = _chain(D, n, stretched)
    perm = np.random.default_rng(90 + D).permutation(n)
    shuffled = np.ascontiguousarray(pos[perm])                # point i of the cloud is point perm[i] of the chain
    sizes = [50] if D == 1 else [20, 18, 16]
    want = _check(fi, _both(fi, sizes, shuffled), shuffled, D, 1.0, 1)
    if not stretched:
        assert not want[0].any() and want[2] == {"clusters": 1, "core": n, "border": 0, "noise": 0, "non_finite": 0}
    else:
        assert want[2]["clusters"] == 2 and want[0][0] == 0   # numbered by their lowest index: point 0's cluster is 0
        assert np.array_equal(want[0] == want[0][0], (perm < short) == (perm[0] < short))


def test_duplicates_count_and_join(fi):
    rng = np.random.default_rng(7)
    sizes = [20, 18, 16]
    noise = rng.uniform(0, 15, size=(200, 3)).astype(np.float32)
    pos = np.concatenate([np.tile(np.float32([[4.5, 6.25, 3.0]]), (40, 1)), noise])[rng.permutation(240)]
    indices = _both(fi, sizes, pos)
    labels, core, stats = _check(fi, indices, pos, 3, 0.0, 40)          # only the copies reach 40, at distance 0
    copies = np.all(pos == np.float32([4.5, 6.25, 3.0]), axis=1)
    assert np.array_equal(core.astype(bool), copies) and np.array_equal(labels == 0, copies) and np.all(labels[~copies] == -1)
    assert stats == {"clusters": 1, "core": 40, "border": 0, "noise": 200, "non_finite": 0}
    assert _check(fi, indices, pos, 3, 0.0, 41)[2]["clusters"] == 0
    _check(fi, indices, pos, 3, 0.5, 41)                                # border points around the copies, if any
    _check(fi, indices, pos, 3, 0.0, 1)                                 # every point its own cluster but the copies


def test_a_border_tie_goes_to_the_lower_core_index(fi):
    for b_first in (True, False):
        pos, by_hand = KR.tie_cloud(b_first)
        for index in _both(fi, [50], pos):
            labels, core, stats = index.cluster(1.0, 4, core=True, stats=True)
            assert np.array_equal(labels, by_hand) and list(core) == [1, 1, 0, 1, 1, 1, 1, 1, 1]
            assert stats == {"clusters": 2, "core": 8, "border": 1, "noise": 0, "non_finite": 0}
        _check(fi, [], pos, 1, 1.0, 4)


@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "%dD" % len(s))
def test_noise_only(fi, sizes):
    D = len(sizes)
    rng = np.random.default_rng(33 + D)
    pos = np.stack([rng.uniform(0, s - 1, 300) for s in sizes], 1).astype(np.float32)
    for index in _both(fi, sizes, pos):
        labels, core, stats = index.cluster(0.5, 400, core=True, stats=True)   # more than the cloud holds
        assert np.all(labels == -1) and not core.any()
        assert stats == {"clusters": 0, "core": 0, "border": 0, "noise": 300, "non_finite": 0}
    _check(fi, _both(fi, sizes, pos), pos, D, 0.5, 400)
    assert fi.cluster_measure(pos, np.full(300, -1, np.int32)) == []
    empty = fi.PointIndex(np.zeros((0, D), np.float32), ndim=D).cluster(1.0, 1, core=True, stats=True)
    assert len(empty[0]) == 0 and len(empty[1]) == 0 and empty[2]["clusters"] == 0


@pytest.mark.parametrize("sizes", [[64], [33, 21], [17, 13, 11]], ids=lambda s: "%dD" % len(s))
def test_non_finite_points(fi, sizes):
    rng = np.random.default_rng(5)
    D = len(sizes)
    pos = np.stack([rng.uniform(0, s - 1, 1000) for s in sizes], 1).astype(np.float32)
    pos[::7, 0] = np.nan
    pos[3::11, D - 1] = np.inf
    pos[5::13, 0] = -np.inf
    bad = ~np.all(np.isfinite(pos), axis=1)
    nn = _median_nn(pos, D)
    indices = _both(fi, sizes, pos)
    for eps, least in ((nn, 1), (2 * nn, 3), (3 * nn, 6)):
        labels, core, stats = _check(fi, indices, pos, D, eps, least)
        assert np.all(labels[bad] == -1) and not core[bad].any() and stats["non_finite"] == bad.sum()
    allbad = np.full((10, D), np.nan, np.float32)
    for index in _both(fi, sizes, allbad):
        labels, stats = index.cluster(1.0, 1, stats=True)
        assert np.all(labels == -1) and stats == {"clusters": 0, "core": 0, "border": 0, "noise": 0, "non_finite": 10}
    # a chain that passes near non-finite points stays whole
    chain, _ = _chain(3, 600, False)
    mixed = np.concatenate([chain, np.full((60, 3), np.nan, np.float32), np.float32([[np.inf, 1, 1]] * 10)])[rng.permutation(670)]
    labels, _, stats = _check(fi, _both(fi, [20, 18, 16], mixed), mixed, 3, 1.0, 1)
    assert stats == {"clusters": 1, "core": 600, "border": 0, "noise": 0, "non_finite": 70}


def test_the_table(fi):
    from field_interpolation_amd import _capi
    rng = np.random.default_rng(12)
    sizes = [1, 256, 257, 600, 0]                             # one member, a chunk, a chunk and one, three chunks, none
    labels = np.concatenate([np.full(m, c, np.int32) for c, m in enumerate(sizes)] + [np.full(50, -1, np.int32)])
    labels = labels[rng.permutation(len(labels))]
    core = rng.integers(0, 2, size=len(labels)).astype(np.uint8)
    for D in (1, 2, 3):
        pos = (rng.normal(size=(len(labels), D)) * [3.0, 40.0, 1e-3][:D] + [0.0, -7.0, 1e4][:D]).astype(np.float32)
        for flags in (core, None):
            rows = fi.cluster_measure(pos, labels, flags, num_clusters=5)
            _same_rows(rows, KR.measure(pos, D, labels, flags, 5), D, (D, flags is None))
        assert [r["count"] for r in rows] == sizes and [r["core"] for r in rows] == [0] * 5
        _same_rows(fi.cluster_measure(pos, labels, core.astype(bool)), KR.measure(pos, D, labels, core, 4), D)
        if D == 1:
            _same_rows(fi.cluster_measure(pos[:, 0].copy(), labels, core), KR.measure(pos, D, labels, core, 4), D)
        # the rows as the library writes them: unused axes and the cluster without a member are zeros
        raw = (_capi.FiClusterRow * 5)()
        ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        assert _capi.lib().fi_cluster_measure(D, len(labels), ptr(pos), ptr(labels), None, 5, raw, 0) == 0
        for r in raw:
            assert list(r.lo[D:]) + list(r.hi[D:]) + list(r.centroid[D:]) == [0.0] * (3 * (3 - D))
        assert bytes(raw[4]) == bytes(C.sizeof(_capi.FiClusterRow))
        # a label out of range, above and below
        for bad in (5, -2):
            spoiled = labels.copy()
            spoiled[len(labels) // 2] = bad
            with pytest.raises(fi.FiError) as e:
                fi.cluster_measure(pos, spoiled, num_clusters=5)
            assert e.value.code == 1
        with pytest.raises(fi.FiError) as e:
            fi.cluster_measure(pos, labels, num_clusters=3)
        assert e.value.code == 1
    keep = fi.keep_clusters(rows, largest=2)
    assert list(keep) == [False, False, True, True, False] and list(fi.keep_clusters(rows, min_points=256)) == [False, True, True, True, False]
    assert list(fi.keep_clusters(rows, largest=1, min_points=601)) == [False] * 5 and list(KR.keep(rows, largest=2)) == list(keep)


def test_repeated_calls_return_the_same_bytes(fi):
    rng = np.random.default_rng(44)
    pos = rng.integers(0, 12, size=(6000, 3)).astype(np.float32)       # many ties and many unions on the same roots
    index = fi.PointIndex(pos)
    first = index.cluster(1.0, 3, core=True, stats=True)
    for again in (index.cluster(1.0, 3, core=True, stats=True), index.cluster(1.0, 3, core=True, stats=True),
                  fi.PointIndex(pos.copy()).cluster(1.0, 3, core=True, stats=True)):
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and first[2] == again[2]
    rows = fi.cluster_measure(pos, first[0], first[1])
    _same_rows(fi.cluster_measure(pos, first[0], first[1]), rows, 3)


def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    f = _field(fi, [10, 10, 10], np.ones((4, 3), np.float32))
    q = np.ones((4, 3), np.float32)
    labels = np.empty(4, np.int32)
    core = np.empty(4, np.uint8)
    stats = _capi.FiClusterStats()
    rows = (_capi.FiClusterRow * 2)()
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    h = C.c_void_p()
    assert L.fi_points_create(C.byref(h), 3, 4, ptr(q), 0) == 0
    try:
        for call, handle in ((L.fi_cluster, f._h), (L.fi_points_cluster, h)):
            assert call(handle, 1.0, 1, ptr(labels), ptr(core), C.byref(stats), 0) == 0
            assert list(labels) == [0] * 4 and list(core) == [1] * 4 and stats.clusters == 1 and stats.core == 4
            assert call(handle, 1.0, 1, ptr(labels), None, None, 0) == 0
            assert call(handle, 1.0, 5, None, None, C.byref(stats), 0) == 0 and stats.clusters == 0 and stats.noise == 4
            assert call(handle, 0.0, 1, ptr(labels), None, None, 0) == 0
            assert call(handle, 1.0, 1, None, None, None, 0) == 1
            assert call(handle, 1.0, 1, None, ptr(core), None, 0) == 1
            assert call(handle, math.nan, 1, ptr(labels), None, None, 0) == 1
            assert call(handle, -1.0, 1, ptr(labels), None, None, 0) == 1
            assert call(handle, math.inf, 1, ptr(labels), None, None, 0) == 1
            assert call(handle, 1.0, 0, ptr(labels), None, None, 0) == 1
            assert call(handle, 1.0, 1, ptr(labels), None, None, 7) == 1
        assert L.fi_points_cluster(None, 1.0, 1, ptr(labels), None, None, 0) == 1
        labels[:] = [0, 1, 1, -1]

        def measure(ndim=3, n=4, pos=ptr(q), lab=ptr(labels), nc=2, out=rows, mem=0):
            return L.fi_cluster_measure(ndim, n, pos, lab, None, nc, out, mem)
        assert measure() == 0 and [rows[0].count, rows[1].count] == [1, 2]
        assert measure(ndim=0) == 1 and measure(ndim=4) == 1 and measure(n=-1) == 1 and measure(nc=-1) == 1
        assert measure(pos=None) == 1 and measure(lab=None) == 1 and measure(out=None) == 1 and measure(mem=3) == 1
        assert measure(nc=1) == 1                                           # the label 1 lies outside [-1, 1)
        assert measure(n=1 << 31) == 5 and measure(nc=1 << 31) == 5
        assert measure(n=0, pos=None, lab=None) == 0 and rows[0].count == 0
        assert measure(nc=0, out=None) == 1                                 # labels 0 and 1 with no cluster at all
    finally:
        L.fi_points_destroy(h)
    with pytest.raises(ValueError):
        fi.cluster_measure(q, labels[:3])
    with pytest.raises(ValueError):
        fi.keep_clusters([], largest=-1)
    s = fi.LatticeField([12, 10, 16], dtype="f32", rank=1, nranks=2)     # a slab context
    s.add_field_constraints(fi.Weights())
    s.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, np.array([[3.0, 4.0, 9.0]], np.float32))
    with pytest.raises(fi.FiError) as e:
        s.cluster(1.0)
    assert e.value.code == 5


def test_batches_of_a_context(fi):
    sizes = [24, 20, 18]
    rng = np.random.default_rng(9)
    a, b = (np.stack([rng.uniform(0, s - 1, n) for s in sizes], 1).astype(np.float32) for n in (700, 300))
    f = _field(fi, sizes, a, b)
    f.add_border_prior(0.5)                                  # lattice points, not data: no part of the set
    ab = np.concatenate([a, b])
    _check(fi, [f], ab, 3, 1.5, 3)
    f.clear_points()
    assert len(f.cluster(1.0)) == 0


def _same_f32(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_clean_points_cuts_the_clump_the_outlier_rules_keep(fi):
    pos, clump = KR.clump_cloud(4)
    rng = np.random.default_rng(70)
    nrm = rng.normal(size=pos.shape).astype(np.float32)
    val = rng.normal(size=len(pos)).astype(np.float32)
    # neither outlier rule removes the 30 ...
    index = fi.PointIndex(pos)
    assert index.statistical_outliers(8, 1.0)[0][clump].all() and index.radius_outliers(1.5, 2)[0][clump].all()
    # ... and the largest cluster is everything else
    got = fi.clean_points(pos, nrm, val, cluster_eps=1.5, largest=1)
    for g, w in zip(got[:3], (pos[~clump], nrm[~clump], val[~clump])):
        _same_f32(g, w)
    assert got[3] == {"input": 1530, "cluster": 30, "output": 1500,
                      "clusters": {"clusters": 2, "core": 1530, "border": 0, "noise": 0, "non_finite": 0}}
    assert fi.clean_points(pos, cluster_eps=1.5, min_cluster=31)[3]["cluster"] == 30
    assert fi.clean_points(pos, cluster_eps=1.5, min_cluster=30)[3]["cluster"] == 0
    # with every step: the same steps by hand on the device, and their restatements
    args = dict(cell=0.5, radius=1.5, min_neighbours=2, k=8, std_ratio=1.0)
    full = fi.clean_points(pos, nrm, val, cluster_eps=1.5, cluster_min_points=3, largest=1, **args)
    p, n, v = fi.thin_points(pos, 0.5, nrm, val)
    keep = fi.PointIndex(p).radius_outliers(1.5, 2)[0]
    p, n, v = p[keep], n[keep], v[keep]
    keep = fi.PointIndex(p).statistical_outliers(8, 1.0)[0]
    p, n, v = p[keep], n[keep], v[keep]
    labels, stats = fi.PointIndex(p).cluster(1.5, 3, stats=True)
    chosen = fi.keep_clusters(fi.cluster_measure(p, labels), largest=1)
    keep = (labels >= 0) & chosen[np.maximum(labels, 0)]
    for g, w in zip(full[:3], (p[keep], n[keep], v[keep])):
        _same_f32(g, w)
    assert full[3]["cluster"] == int((~keep).sum()) and full[3]["clusters"] == stats and full[3]["output"] == int(keep.sum())
    wp, wn, wv, wreport = CR.clean(pos, 3, nrm, val, **args)
    wl, _, wstats = KR.cluster(wp, 3, 1.5, 3)
    wkeep = KR.keep(KR.measure(wp, 3, wl, None, wstats["clusters"]), largest=1)
    wkeep = (wl >= 0) & wkeep[np.maximum(wl, 0)]
    for g, w in zip(full[:3], (wp[wkeep], wn[wkeep], wv[wkeep])):
        _same_f32(g, w)
    # without cluster_eps: what the function returned before it had the step -- its steps composed by hand
    plain = fi.clean_points(pos, nrm, val, **args)
    for g, w in zip(plain[:3], (p, n, v)):
        _same_f32(g, w)
    stats_before = plain[3].pop("stats")
    assert plain[3] == {k: wreport[k] for k in ("input", "thinned", "radius", "statistical", "output")}
    assert stats_before["kept"] == len(p) and set(plain[3]) == {"input", "thinned", "radius", "statistical", "output"}
    labels, rows = fi.cluster_points(pos, 1.5, measure=True)
    assert np.array_equal(labels, fi.cluster_points(pos, 1.5)) and sorted(r["count"] for r in rows) == [30, 1500]


def test_device_tensors(tmp_path):
    """torch device tensors in, torch device tensors out, equal to the restatement; in a fresh process
    (tests/cluster_torch_worker.py), as torch must stay out of this one"""
    pos, clump = KR.clump_cloud(3)
    np.savez(tmp_path / "in.npz", pos=pos)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cluster_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"].all()
    want = KR.cluster(pos, 3, 0.6, 4)
    rows = KR.measure(pos, 3, want[0], want[1], want[2]["clusters"])
    for ours in ("pts", "ctx"):
        assert o[ours + "_labels"].dtype == np.int32 and np.array_equal(o[ours + "_labels"], want[0])
        assert np.array_equal(o[ours + "_core"], want[1].astype(bool))
        assert list(o[ours + "_stats"]) == [want[2][k] for k in ("clusters", "core", "border", "noise", "non_finite")]
    assert list(o["count"]) == [r["count"] for r in rows] and list(o["cores"]) == [r["core"] for r in rows]
    for key, kind in (("lo", np.uint32), ("hi", np.uint32), ("centroid", np.uint64)):
        assert np.array_equal(o[key].view(kind), np.stack([r[key] for r in rows]).view(kind)), key
    assert np.array_equal(o["labels_only"], KR.cluster(pos, 3, 1.5)[0])
    _same_f32(o["clean_pos"], pos[~clump])
