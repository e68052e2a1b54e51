"""tests/cluster_reference.py, the numpy restatement of the clustering contract (include/fi_hip.h fi_cluster),
against answers known by hand: what the GPU tests hold the device to must itself be right.  No device, no library."""
import numpy as np
import pytest

import cloud_reference as CR
import cluster_reference as KR


def _square(x0, y0, side=3):
    g = np.arange(side, dtype=np.float32)
    return np.stack([np.repeat(g, side) + x0, np.tile(g, side) + y0], 1)


def test_two_lattice_squares_a_gap_of_two_apart():
    pos = np.concatenate([_square(0, 0), _square(4, 0)])      # x = 0..2 and x = 4..6: the gap is 2
    labels, core, stats = KR.cluster(pos, 2, 1.0)
    assert list(labels) == [0] * 9 + [1] * 9 and core.all()
    assert stats == {"clusters": 2, "core": 18, "border": 0, "noise": 0, "non_finite": 0}
    labels, _, stats = KR.cluster(pos, 2, 2.0)
    assert not labels.any() and stats["clusters"] == 1
    labels, _, stats = KR.cluster(pos, 2, float(np.nextafter(np.float32(2.0), np.float32(0))))
    assert stats["clusters"] == 2                             # one float below the gap: not joined
    # numbered by the lowest core index, not by position
    swapped = np.concatenate([_square(4, 0), _square(0, 0)])
    assert list(KR.cluster(swapped, 2, 1.0)[0]) == [0] * 9 + [1] * 9


def test_a_line_of_ten_points():
    pos = np.arange(10, dtype=np.float32).reshape(-1, 1)
    labels, core, stats = KR.cluster(pos, 1, 1.0, 3)          # an end point has itself and one neighbour
    assert list(core) == [0] + [1] * 8 + [0] and not labels.any()
    assert stats == {"clusters": 1, "core": 8, "border": 2, "noise": 0, "non_finite": 0}
    labels, core, stats = KR.cluster(pos, 1, 1.0, 4)
    assert not core.any() and np.all(labels == -1)
    assert stats == {"clusters": 0, "core": 0, "border": 0, "noise": 10, "non_finite": 0}
    labels, core, stats = KR.cluster(pos, 1, 1.0, 1)
    assert core.all() and not labels.any() and stats["clusters"] == 1


def test_a_border_point_between_two_clusters_goes_to_the_lower_core_index():
    for b_first in (True, False):
        pos, by_hand = KR.tie_cloud(b_first)
        labels, core, stats = KR.cluster(pos, 1, 1.0, 4)
        assert list(core) == [1, 1, 0, 1, 1, 1, 1, 1, 1]
        assert list(labels) == list(by_hand) and labels[2] == labels[1] != labels[3]
        # the border point reaches both clusters and joins neither to the other
        assert stats == {"clusters": 2, "core": 8, "border": 1, "noise": 0, "non_finite": 0}
    # the nearer core point wins whatever its index: B's near point moved to 0.5, behind A's in index
    pos = np.float32([-2.0, -1.0, 0.0, 0.5, -1.5, -1.75, 1.25, 1.375, 1.5]).reshape(-1, 1)
    labels, core, _ = KR.cluster(pos, 1, 1.0, 4)
    assert list(core) == [1, 1, 0, 1, 1, 1, 1, 1, 1] and list(labels) == [0, 0, 1, 1, 0, 0, 1, 1, 1]


def test_duplicates_count_and_non_finite_points_are_noise():
    pos = np.float32([[1, 1], [1, 1], [1, 1], [np.nan, 0], [5, 5], [np.inf, 1]])
    labels, core, stats = KR.cluster(pos, 2, 0.0, 3)          # eps = 0: only duplicates are within reach
    assert list(labels) == [0, 0, 0, -1, -1, -1] and list(core) == [1, 1, 1, 0, 0, 0]
    assert stats == {"clusters": 1, "core": 3, "border": 0, "noise": 1, "non_finite": 2}
    empty = KR.cluster(np.zeros((0, 3), np.float32), 3, 1.0)
    assert empty[0].size == 0 and empty[2]["clusters"] == 0
    with pytest.raises(ValueError):
        KR.cluster(pos, 2, np.inf)
    with pytest.raises(ValueError):
        KR.cluster(pos, 2, 1.0, 0)


def test_against_scipy_connected_components():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    import nearest_reference as NR
    rng = np.random.default_rng(3)
    for D in (1, 2, 3):
        pos = rng.uniform(0, 12, size=(400, D)).astype(np.float32)
        eps = [0.02, 0.5, 1.2][D - 1]
        graph = sp.csr_matrix(np.sqrt(NR.sq_dist(pos, pos)) <= np.float32(eps))
        count, comp = connected_components(graph, directed=False)
        labels, core, stats = KR.cluster(pos, D, eps, 1)
        assert stats["clusters"] == count and 1 < count < 400 and core.all()
        first = {}                                            # scipy's components renumbered by their lowest index
        want = np.array([first.setdefault(c, len(first)) for c in comp])
        assert np.array_equal(labels, want)


def test_the_table():
    rng = np.random.default_rng(8)
    pos = rng.uniform(-3, 3, size=(700, 3)).astype(np.float32)
    labels = rng.integers(-1, 3, size=700).astype(np.int32)
    labels[labels == 1] = 0                                   # cluster 1 has no member
    core = rng.integers(0, 2, size=700).astype(np.uint8)
    rows = KR.measure(pos, 3, labels, core, 3)
    assert [r["count"] for r in rows] == [int((labels == c).sum()) for c in range(3)] and rows[1]["count"] == 0
    assert rows[0]["count"] > 256                             # more than one chunk
    assert not rows[1]["centroid"].any() and not rows[1]["lo"].any()
    for c in (0, 2):
        m = labels == c
        assert rows[c]["core"] == int(core[m].sum())
        assert np.array_equal(rows[c]["lo"], pos[m].min(0)) and np.array_equal(rows[c]["hi"], pos[m].max(0))
        assert np.allclose(rows[c]["centroid"], pos[m].astype(np.float64).mean(0), rtol=1e-13, atol=1e-13)
    assert [r["core"] for r in KR.measure(pos, 3, labels, None, 3)] == [0, 0, 0]
    two = KR.measure(pos[:, :2], 2, labels, None, 3)[0]
    assert two["lo"][2] == 0 and two["hi"][2] == 0 and two["centroid"][2] == 0
    with pytest.raises(ValueError):
        KR.measure(pos, 3, labels, None, 2)
    with pytest.raises(ValueError):
        KR.measure(pos, 3, np.full(700, -2), None, 3)
    assert list(KR.keep(rows, largest=1)) == [rows[0]["count"] >= rows[2]["count"], False, rows[0]["count"] < rows[2]["count"]]
    assert list(KR.keep(rows, min_points=1)) == [True, False, True]


def test_the_planted_clump_survives_both_outlier_rules_and_not_the_clusters():
    """the fixture of test_gpu_cluster.py's clean_points test, on the restatements alone"""
    pos, clump = KR.clump_cloud(4)
    assert clump.sum() == 30 and len(pos) == 1530
    assert CR.radius_outliers(pos, 3, 1.5, 2).astype(bool)[clump].all()
    assert CR.statistical_outliers(pos, 3, 8, 1.0)[0].astype(bool)[clump].all()
    labels, _, stats = KR.cluster(pos, 3, 1.5)
    rows = KR.measure(pos, 3, labels, None, stats["clusters"])
    keep = KR.keep(rows, largest=1)
    assert np.array_equal(keep[labels], ~clump)               # the largest cluster is everything but the 30
    assert sorted(r["count"] for r in rows) == [30, 1500]
