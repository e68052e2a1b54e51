"""The nearest-point oracle (tests/nearest_reference.py) on the CPU: against scipy's cKDTree on random clouds, and on hand
cases of the contract's rules -- ties, non-finite points and queries, an empty set, points outside the lattice, 1-D,
max_distance, the lattice order of the distance field."""
import numpy as np
import pytest

import nearest_reference as R


@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_matches_a_kd_tree_on_random_clouds(ndim):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(10 + ndim)
    P = rng.uniform(-5, 60, size=(3000, ndim)).astype(np.float32)
    Q = rng.uniform(-20, 80, size=(2000, ndim)).astype(np.float32)
    d, i = R.nearest(P, Q, ndim)
    kd, _ = cKDTree(P.astype(np.float64)).query(Q.astype(np.float64))
    np.testing.assert_allclose(d, kd, rtol=1e-5, atol=1e-5)
    # the index the oracle returns is a nearest point by the exact distance as well (to fp32 rounding)
    exact = np.linalg.norm(P[i].astype(np.float64) - Q.astype(np.float64), axis=1)
    np.testing.assert_allclose(exact, kd, rtol=1e-5, atol=1e-5)
    assert d.dtype == np.float32 and i.dtype == np.int64


def test_ties_take_the_smallest_index():
    P = np.array([[3, 0], [1, 0], [2, 1], [1, 0], [2, -1]], np.float32)   # (2, 0) is 1 from points 0, 1, 2, 3, 4
    d, i = R.nearest(P, np.array([[2, 0], [1, 0], [5, 0]], np.float32), 2)
    assert list(i) == [0, 1, 0]
    assert list(d) == [1.0, 0.0, 2.0]


def test_every_point_identical():
    P = np.full((50, 3), 7.25, np.float32)
    d, i = R.nearest(P, np.array([[7.25, 7.25, 7.25], [0, 0, 0]], np.float32), 3)
    assert list(i) == [0, 0]
    assert d[0] == 0.0 and d[1] == np.sqrt(np.float32(3 * 7.25 ** 2))


def test_non_finite_points_are_never_nearest_and_non_finite_queries_give_nan():
    P = np.array([[np.nan, 0], [0, np.inf], [-np.inf, 1], [4, 4], [5, 5]], np.float32)
    Q = np.array([[0, 0], [np.nan, 1], [1, np.inf], [5, 5]], np.float32)
    d, i = R.nearest(P, Q, 2)
    assert i[0] == 3 and d[0] == np.sqrt(np.float32(32))
    assert np.isnan(d[1]) and i[1] == -1
    assert np.isnan(d[2]) and i[2] == -1
    assert i[3] == 4 and d[3] == 0
    d, i = R.nearest(P[:3], Q, 2)                      # no finite point at all
    assert np.isinf(d[0]) and i[0] == -1 and np.isnan(d[1])


def test_an_empty_set():
    d, i = R.nearest(np.zeros((0, 3), np.float32), np.ones((4, 3), np.float32), 3)
    assert np.all(np.isinf(d)) and np.all(i == -1)
    d, i = R.nearest(np.ones((4, 3), np.float32), np.zeros((0, 3), np.float32), 3)
    assert d.shape == (0,) and i.shape == (0,)


def test_points_outside_the_lattice_count():
    P = np.array([[-40, -40], [1e4, 3]], np.float32)
    d, i = R.distance_field(P, [4, 3])
    assert np.all(i == 0)
    assert d[0] == np.sqrt(np.float32(3200))


def test_one_dimension_and_max_distance():
    P = np.array([[5.0], [9.0], [1.0]], np.float32)
    Q = np.array([[6.0], [7.0], [0.0], [20.0]], np.float32)
    d, i = R.nearest(P, Q, 1)
    assert list(i) == [0, 0, 2, 1] and list(d) == [1, 2, 1, 11]          # (7: 2 from points 0 and 1 -> 0)
    d, i = R.nearest(P, Q, 1, max_distance=1.0)
    assert list(i) == [0, -1, 2, -1] and np.isinf(d[1]) and np.isinf(d[3])
    d, i = R.nearest(P, Q, 1, max_distance=0.0)
    assert np.all(i == -1)
    d, i = R.nearest(P, P, 1, max_distance=0.0)
    assert list(i) == [0, 1, 2] and np.all(d == 0)


def test_overflowing_sums_keep_their_index_unless_max_distance_is_finite():
    P = np.array([[3e38, 0], [-3e38, 0]], np.float32)
    d, i = R.nearest(P, np.array([[-3e38, 0], [0, 0]], np.float32), 2)
    assert i[0] == 1 and d[0] == 0
    assert np.isinf(d[1]) and i[1] == 0            # every s is +inf: the smallest index
    d, i = R.nearest(P, np.array([[0, 0]], np.float32), 2, max_distance=1e30)
    assert np.isinf(d[0]) and i[0] == -1


def test_the_distance_field_runs_x_fastest():
    P = np.array([[0, 0, 0], [3, 1, 2]], np.float32)
    d, i = R.distance_field(P, [4, 2, 3])
    assert d.shape == (24,)
    assert i[0] == 0 and i[3 + 4 * 1 + 8 * 2] == 1
    q = R.lattice_points([4, 2, 3])
    assert list(q[1]) == [1, 0, 0] and list(q[4]) == [0, 1, 0] and list(q[8]) == [0, 0, 1]


def test_chunking_does_not_change_the_result():
    rng = np.random.default_rng(4)
    P = rng.integers(0, 6, size=(500, 2)).astype(np.float32)        # many ties
    Q = rng.integers(-2, 8, size=(300, 2)).astype(np.float32)
    a = R.nearest(P, Q, 2)
    b = R.nearest(P, Q, 2, chunk_pairs=7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
