"""The numpy restatement of the normal-orientation contract (tests/orient_reference.py; include/fi_hip.h
fi_orient_normals) against clouds worked out by hand, and what the contract is for: on closed shapes the
propagated normals all look outward, where the canonical sign of estimate_normals is right for every second one.  No GPU."""
import functools

import numpy as np

import normals_reference as R
import orient_reference as O
from util import sphere_points

Z = np.float32(-0.0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_six_points_by_hand():
    """two triangles' worth of points, 1.5 apart at most inside a group: k = 3 lists everybody inside a group.
    Group A = {0, 1, 2}: d01 = -0.5, d02 = -0.25, d12 = 0.125 - 1 = -0.875, all flips; by a descending the forest is
    {1,2}, {0,1} and {0,2} closes a cycle (an odd one: no signs satisfy all three edges).  t = (+, -, +); the highest point
    is 2 and t_2 n_2 = (-0.25, -1) looks down: S = -1.
    Group B = {3, 4, 5}: {3,4} d = -1 (flip), {4,5} d = 0 (a = 0, no flip), 3-5 are 2.02 apart.  t = (+, -, -); the highest
    point is 5 and t_5 n_5 = (-0, -1): S = -1."""
    pos = np.array([[0, 0], [1, 0], [0.5, 0.8], [10, 0], [11, 0], [12, 0.25]], np.float32)
    nrm = np.array([[1, 0], [-0.5, 1], [-0.25, -1], [1, 0], [-1, 0], [0, 1]], np.float32)
    got, comp = O.orient_normals(pos, nrm, 2, 3, max_distance=1.5)
    want = np.array([[-1, Z], [-0.5, 1], [0.25, 1], [-1, Z], [-1, 0], [0, 1]], np.float32)
    assert np.array_equal(_bits(got), _bits(want)), got
    assert comp.tolist() == [0, 0, 0, 3, 3, 3]
    live = O.live_points(pos, nrm)
    lo, hi, a, flip = O.edges(nrm, R.knn(pos, pos, 2, 3, 1.5)[1], live)
    assert list(zip(lo.tolist(), hi.tolist())) == [(3, 4), (1, 2), (0, 1), (0, 2), (4, 5)]
    assert a.tolist() == [1.0, 0.875, 0.5, 0.25, 0.0] and flip.tolist() == [True, True, True, True, False]
    assert O.forest_signs(6, lo, hi, flip)[2].tolist() == [True, True, True, False, True]
    # a viewpoint high above x = 11: in A the votes w(t n) are (+, -, -) -> S = -1 as before; in B point 3 votes +, point 4
    # has w = 0 and does not vote, point 5 votes -: a tie, so the extreme rule decides as before
    got_v, _ = O.orient_normals(pos, nrm, 2, 3, max_distance=1.5, viewpoints=np.array([[11.0, 1000.0]], np.float32))
    assert np.array_equal(_bits(got_v), _bits(want))
    # one far below: A votes (+, +, +), B votes (+, none, +)
    got_b, _ = O.orient_normals(pos, nrm, 2, 3, max_distance=1.5, viewpoints=np.array([[11.0, -1000.0]], np.float32))
    assert np.array_equal(_bits(got_b), _bits(-want))
    # dead points: a NaN position, a zero normal, a NaN normal keep their bits; 0-1 is all that is left
    pos2, nrm2 = pos.copy(), nrm.copy()
    pos2[2, 0] = np.nan
    nrm2[4] = 0
    nrm2[5, 1] = np.nan
    got2, comp2 = O.orient_normals(pos2, nrm2, 2, 3, max_distance=1.5)
    assert comp2.tolist() == [0, 0, -1, 3, -1, -1]
    # A: t = (+, -), the highest (a tie at y = 0: index 0) has n = (1, 0): axis 1 is zero, axis 0 decides: S = +1
    want2 = nrm2.copy()
    want2[1] = [0.5, -1]
    assert np.array_equal(_bits(got2), _bits(want2))


def test_an_edge_listed_from_one_side_only_is_in_the_forest():
    """on a line at x = 0, 1, 1.9, 4 with k = 2 (itself and one more): 0 lists 1, 1 lists 2, 2 lists 1, 3 lists 2 -- the
    edges {0,1} and {2,3} are known from one end only, and without them there would be three components"""
    pos = np.array([[0, 0], [1, 0], [1.9, 0], [4, 0]], np.float32)
    nrm = np.array([[0, 1], [0, -1], [0, 1], [0, -2]], np.float32)
    idx = R.knn(pos, pos, 2, 2)[1]
    assert idx.tolist() == [[0, 1], [1, 2], [2, 1], [3, 2]]
    lo, hi, a, flip = O.edges(nrm, idx, O.live_points(pos, nrm))
    assert list(zip(lo.tolist(), hi.tolist())) == [(2, 3), (0, 1), (1, 2)] and a.tolist() == [2.0, 1.0, 1.0]
    assert O.forest_signs(4, lo, hi, flip)[2].all()
    got, comp = O.orient_normals(pos, nrm, 2, 2)
    assert comp.tolist() == [0, 0, 0, 0]
    # t = (+, -, +, -); every y is 0, so the extreme point is 0 and looks up: S = +1
    assert np.array_equal(_bits(got), _bits(np.array([[0, 1], [Z, 1], [0, 1], [Z, 2]], np.float32)))


@functools.lru_cache(maxsize=None)
def _case(sizes, n, k, noise, seed):
    """(pos, centre, canonical normals, neighbours, propagated normals, components)"""
    D = len(sizes)
    pos, _ = sphere_points(np.random.default_rng(seed), list(sizes), n, noise=noise)
    nb = R.knn(pos, pos, D, k)
    nrm = R.estimate_normals(pos, D, k, neighbours=nb)[0]
    out, comp = O.orient_normals(pos, nrm, D, k, neighbours=nb)
    centre = ((np.array(sizes) - 1) / 2.0).astype(np.float32)
    for a in (pos, nrm, out, comp):
        a.setflags(write=False)
    return pos, centre, nrm, nb, out, comp


def _outward(nrm, pos, centre):
    return float(np.mean(np.sum(nrm.astype(np.float64) * (pos - centre), axis=1) > 0))


def _quality(sizes, n, k, noise, seed):
    pos, centre, nrm, _, out, comp = _case(sizes, n, k, noise, seed)
    share, before = _outward(out, pos, centre), _outward(nrm, pos, centre)
    print("outward: %.4f propagated, %.4f canonical; %d components" % (share, before, np.unique(comp).size))
    assert 0.4 < before < 0.6                                          # the canonical sign: a coin toss
    assert np.unique(comp).size == 1 and comp[0] == 0
    assert np.array_equal(np.abs(out), np.abs(nrm))                    # signs only
    return share


def test_sphere_noiseless():
    assert _quality((20, 18, 16), 4000, 16, 0.0, 1) >= 0.99            # measured for this seed: 1.0000


def test_sphere_noisy():
    assert _quality((20, 18, 16), 4000, 16, 0.05, 2) >= 0.99           # measured for this seed: 1.0000


def test_sphere_sparse():
    assert _quality((20, 18, 16), 600, 8, 0.0, 3) >= 0.99              # measured for this seed: 1.0000


def test_circle():
    assert _quality((40, 30), 4000, 16, 0.0, 4) >= 0.99                # measured for this seed: 1.0000


def test_the_vote_decides_the_components_sign():
    sizes = (20, 18, 16)
    pos, centre, nrm, nb, out, _ = _case(sizes, 4000, 16, 0.0, 1)
    far = (centre + np.array([500.0, 0, 0], np.float32)).reshape(1, 3)
    seen, _ = O.orient_normals(pos, nrm, 3, 16, neighbours=nb, viewpoints=far)
    assert _outward(seen, pos, centre) == 1.0                          # the far side too, where the per-point test fails
    per_point = R.estimate_normals(pos, 3, 16, neighbours=nb, viewpoints=far)[0]
    assert 0.4 < _outward(per_point, pos, centre) < 0.6
    inside, _ = O.orient_normals(pos, nrm, 3, 16, neighbours=nb, viewpoints=centre.reshape(1, 3))
    assert _outward(inside, pos, centre) == 0.0
    assert np.array_equal(_bits(inside), _bits(-seen))
    along, _ = O.orient_normals(pos, nrm, 3, 16, neighbours=nb, directions=(centre - pos).astype(np.float32))
    assert np.array_equal(_bits(along), _bits(inside))
    blind, _ = O.orient_normals(pos, nrm, 3, 16, neighbours=nb, viewpoints=np.full((4000, 3), np.nan, np.float32))
    assert np.array_equal(_bits(blind), _bits(out))                    # nobody votes: the extreme rule
