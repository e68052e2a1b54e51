"""The numpy restatement of the point-cloud cleaning contract (tests/cloud_reference.py; include/fi_hip.h fi_radius_count ..
fi_cloud_thin) held to facts known without it: an fp64 brute force, normals_reference.knn with the point
itself taken out, math.fsum, thinning that must return its input, means computed by hand -- and the pipeline's worth on a
scan with planted stray points.  No GPU.  The figures measured with the restatement stand in the tests that state them (and in
DESIGN.md 4.19)."""
import functools
import math

import numpy as np

import cloud_reference as CR
import normals_reference as N


def test_radius_count_equals_an_fp64_brute_force_away_from_the_radius():
    rng = np.random.default_rng(11)
    for D in (1, 2, 3):
        P = rng.uniform(0, 10, size=(400, D)).astype(np.float32)
        Q = rng.uniform(-1, 11, size=(150, D)).astype(np.float32)
        d = np.sqrt(((P[None].astype(np.float64) - Q[:, None].astype(np.float64)) ** 2).sum(axis=2))
        radius = 1.75
        ok = np.all(np.abs(d - radius) >= 1e-3, axis=1)      # fp32 and fp64 agree on which side of the radius a pair lies
        assert ok.sum() > 30
        want = (d <= radius).sum(axis=1)
        got = CR.radius_count(P, Q, D, radius)
        assert got.dtype == np.int32 and np.array_equal(got[ok], want[ok])
        assert np.array_equal(CR.radius_count(P, Q, D, radius, limit=3)[ok], np.minimum(want, 3)[ok])
        assert np.all(CR.radius_count(P, Q, D, np.inf) == len(P))
    Q = np.array([[np.nan, 0.0], [0.0, np.inf], [1.0, 1.0]], np.float32)
    P = np.array([[1.0, 1.0], [np.nan, 1.0], [1.0, 2.0]], np.float32)
    assert list(CR.radius_count(P, Q, 2, 1.0)) == [-1, -1, 2]   # on the radius counts; the NaN point does not


def test_neighbour_distances_are_the_knn_results_without_the_point_itself():
    rng = np.random.default_rng(12)
    for D in (1, 2, 3):
        P = rng.uniform(0, 20, size=(600, D)).astype(np.float32)
        assert len(np.unique(P, axis=0)) == len(P)           # no duplicates: a point's nearest point is itself, at 0
        for k in (1, 7, 16):
            d, i = N.knn(P, P, D, k + 1)
            assert np.array_equal(i[:, 0], np.arange(len(P)))
            mean, kth, counts = CR.neighbour_distances(P, D, k)
            assert np.all(counts == k)
            assert np.array_equal(kth.view(np.uint32), d[:, k].view(np.uint32))
            acc = np.zeros(len(P))
            for r in range(1, k + 1):
                acc = acc + d[:, r].astype(np.float64)
            assert np.array_equal(mean.view(np.uint32), (acc / k).astype(np.float32).view(np.uint32))


def test_neighbour_distance_rules():
    P = np.array([[0, 0], [0, 0], [3, 4], [np.nan, 0], [100, 100]], np.float32)
    mean, kth, counts = CR.neighbour_distances(P, 2, 2, max_distance=6.0)
    assert list(counts) == [2, 2, 2, 0, 0]                   # a duplicate is a neighbour at 0; the far point has none
    assert list(mean[:3]) == [2.5, 2.5, 5.0] and list(kth[:3]) == [5.0, 5.0, 5.0]
    assert np.isnan(mean[3]) and np.isnan(kth[3]) and np.isinf(mean[4]) and np.isinf(kth[4])
    keep, stats = CR.statistics(mean, 1.0)
    assert stats["counted"] == 3 and list(keep) == [1, 1, 0, 0, 0] and stats["kept"] == 2
    assert abs(stats["mean"] - 10.0 / 3.0) < 1e-15 and abs(stats["stddev"] - math.sqrt(12.5 / 9.0)) < 1e-15
    keep, stats = CR.statistics(np.full(4, np.inf, np.float32), 2.0)
    assert stats == {"counted": 0, "kept": 0, "mean": 0.0, "stddev": 0.0, "threshold": 0.0} and not keep.any()


def test_tree_sum_against_fsum():
    rng = np.random.default_rng(13)
    for n in (1, 255, 256, 257, 3 * 256 + 5, 20000):
        v = rng.uniform(0, 3, n) * 10.0 ** rng.integers(-3, 4, n)
        assert abs(CR.tree_sum(v) - math.fsum(v)) <= 1e-12 * math.fsum(v)


def test_thinning_one_point_a_cell_returns_the_input():
    rng = np.random.default_rng(14)
    for D in (1, 2, 3):
        cells = rng.permutation(40 ** D)[:300]
        c = np.stack([(cells // 40 ** a) % 40 - 20 for a in range(D)], 1)
        P = ((c + rng.uniform(0.05, 0.95, size=c.shape)) * 0.5).astype(np.float32)
        Nm = rng.normal(size=P.shape).astype(np.float32)
        Nm /= np.linalg.norm(Nm, axis=1, keepdims=True).astype(np.float32)
        V = rng.normal(size=len(P)).astype(np.float32)
        for mode in (CR.MEAN, CR.FIRST):
            t = CR.thin(P, D, 0.5, mode=mode, normals=Nm, values=V)
            at = t["indices"]
            assert sorted(at) == list(range(len(P))) and np.all(t["counts"] == 1)
            assert np.array_equal(t["cell_map"][at], np.arange(len(P)))
            assert np.array_equal(t["positions"].view(np.uint32), P[at].view(np.uint32))
            assert np.array_equal(t["values"].view(np.uint32), V[at].view(np.uint32))
            if mode == CR.FIRST:
                assert np.array_equal(t["normals"].view(np.uint32), Nm[at].view(np.uint32))
            else:                                            # renormalised: the same direction, the length's rounding apart
                assert np.abs(t["normals"] - Nm[at]).max() < 2e-7


def test_thinning_an_integer_grid_by_hand():
    g = np.stack(np.meshgrid(np.arange(-2, 2), np.arange(0, 4), indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
    P = np.concatenate([g, [[np.nan, 1.0]], [[-2.0, 0.0]]]).astype(np.float32)     # a NaN point and a duplicate of point 0
    V = np.arange(len(P), dtype=np.float32)
    t = CR.thin(P, 2, 2.0, values=V)
    # cells (x, y) in key order: y is the slower axis -- (-1, 0), (0, 0), (-1, 1), (0, 1)
    assert list(t["counts"]) == [5, 4, 4, 4]
    assert np.array_equal(t["positions"], np.array([[-1.6, 0.4], [0.5, 0.5], [-1.5, 2.5], [0.5, 2.5]], np.float32))
    assert list(t["indices"]) == [0, 8, 2, 10]
    assert list(t["cell_map"]) == [0, 0, 2, 2, 0, 0, 2, 2, 1, 1, 3, 3, 1, 1, 3, 3, -1, 0]
    assert np.array_equal(t["values"], np.array([(0 + 1 + 4 + 5 + 17) / 5, (8 + 9 + 12 + 13) / 4, (2 + 3 + 6 + 7) / 4,
                                                 (10 + 11 + 14 + 15) / 4], np.float32))
    f = CR.thin(P, 2, 2.0, values=V, mode=CR.FIRST, origin=[-2.0, 0.0])
    assert np.array_equal(f["positions"], P[[0, 8, 2, 10]]) and list(f["values"]) == [0, 8, 2, 10]
    N2 = np.tile(np.array([[0.0, 2.0]], np.float32), (len(P), 1))
    N2[[8, 12]] *= -1                                        # cell 1 (points 8, 9, 12, 13): two up, two down -- a zero sum
    assert np.array_equal(CR.thin(P, 2, 2.0, normals=N2)["normals"], np.array([[0, 1], [0, 0], [0, 1], [0, 1]], np.float32))
    try:
        CR.thin(np.array([[3e6, 0.0]], np.float32), 2, 1.0)
        assert False, "2^20 cells from the origin must be refused"
    except ValueError:
        pass
    assert len(CR.thin(np.full((3, 2), np.nan, np.float32), 2, 1.0)["positions"]) == 0


SEED = 2


@functools.lru_cache(maxsize=None)
def planted():
    return CR.planted_cloud(SEED)


def test_the_statistical_rule_removes_the_planted_points_and_no_others():
    """4000 points of a sphere scan (noise 0.05) and 36 stray points at least 2 units from its surface, seed 2.  Measured
    with this restatement: k = 8, std_ratio = 1.0 removes 36 points, all 36 planted ones and no sphere point (mean 0.66248,
    stddev 0.86793, threshold 1.53042); std_ratio = 2.0 removes 34 and 3.0 removes 33 -- two and three stray points that sit
    near one another pass, which is why the test states 1.0.  Seeds 1 and 3 give 36 / 36 / 34 and 36 / 36 / 36."""
    pos, stray = planted()
    keep, stats = CR.statistical_outliers(pos, 3, 8, 1.0)
    keep = keep.astype(bool)
    assert stats["counted"] == 4036 and stats["kept"] == 4000
    assert int((~keep).sum()) == 36 and np.array_equal(~keep, stray)
    mean = CR.neighbour_distances(pos, 3, 8)[0]
    assert int((~CR.statistics(mean, 2.0)[0].astype(bool)).sum()) == 34
    assert int((~CR.statistics(mean, 3.0)[0].astype(bool)).sum()) == 33


def test_the_radius_rule_removes_the_planted_points_and_no_others():
    """the same cloud: radius 1.5 with min_neighbours 2 removes exactly the 36 planted points (measured; seeds 1 and 3 too)"""
    pos, stray = planted()
    keep = CR.radius_outliers(pos, 3, 1.5, 2).astype(bool)
    assert int((~keep).sum()) == 36 and np.array_equal(~keep, stray)
    # the pipeline: the radius stage leaves the sphere, the statistical stage then judges the sphere's points among themselves
    p2, _n, _v, report = CR.clean(pos, 3, radius=1.5, min_neighbours=2, k=8, std_ratio=3.0)
    sphere = pos[~stray]
    keep2 = CR.statistical_outliers(sphere, 3, 8, 3.0)[0].astype(bool)
    assert report["input"] == 4036 and report["radius"] == 36 and report["statistical"] == int((~keep2).sum())
    assert report["output"] == len(p2) and np.array_equal(p2, sphere[keep2])
