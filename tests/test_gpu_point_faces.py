"""The two faces of the point-set operations -- a context's data points (fi_<op>, LatticeField) and a point set of its own
(fi_points_<op>, PointIndex) -- held together: the same points give the same bytes through either face, the same bad
arguments the same status code and fi_last_error text, and a context refuses in this order: arguments, a slab, and only
then (for the queries, after the early return at n = 0) the build of its search structure.  What the results must be is the
business of the units' own tests (test_gpu_nearest.py, _knn, _normals, _orient, _cloud, _cluster, _mls)."""
import math

import numpy as np
import pytest

import point_faces as P

pytestmark = pytest.mark.gpu

SIZES = {2: [12, 10], 3: [12, 10, 9]}
SLAB_TEXT = "nearest points on a slab context: a rank sees only its own points"


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _field(fi, sizes, *batches, **slab):
    f = fi.LatticeField(sizes, **slab)
    f.add_field_constraints(fi.Weights())
    for p in batches:
        f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, p)
    return f


def _cloud(D):
    """300 points near a circle / sphere, one exact duplicate (in the other batch) and one point with a NaN coordinate;
    40 queries around them, one of them non-finite"""
    rng = np.random.default_rng(40 + D)
    d = rng.normal(size=(300, D))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = ((np.array(SIZES[D]) - 1) / 2.0 + 3.5 * d + rng.normal(scale=0.1, size=d.shape)).astype(np.float32)
    pos[200] = pos[17]
    pos[250, 0] = np.nan
    q = np.stack([rng.uniform(-2.0, s + 1.0, 40) for s in SIZES[D]], 1).astype(np.float32)
    q[5, D - 1] = np.inf
    return pos, q


def _bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want, what):
    """every array, dict and number of `got` is `want`'s: floats bit for bit, a NaN where the other has one"""
    assert type(got) is type(want), what
    if isinstance(got, (tuple, list)):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, "%s[%d]" % (what, i))
    elif isinstance(got, dict):
        assert sorted(got) == sorted(want), what
        for key in got:
            _same(got[key], want[key], "%s[%r]" % (what, key))
    elif isinstance(got, np.ndarray):
        assert got.dtype == want.dtype and got.shape == want.shape, what
        if got.dtype.kind == "f":
            assert np.array_equal(np.isnan(got), np.isnan(want)), what
            differ = (_bits(got) != _bits(want)) & ~np.isnan(want)
        else:
            differ = got != want
        bad = np.flatnonzero(differ)
        assert bad.size == 0, (what, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])
    else:
        _same(np.asarray(got), np.asarray(want), what)


@pytest.mark.parametrize("D", [2, 3])
def test_the_same_bytes_from_both_faces(fi, D):
    pos, q = _cloud(D)
    f = _field(fi, SIZES[D], pos[:130], pos[130:])
    pi = fi.PointIndex(pos, ndim=D)
    view = np.float32(np.array(SIZES[D]) * 2.0)
    normals = pi.estimate_normals(k=8)
    calls = [("nearest", dict(queries=q, indices=True)), ("nearest", dict(queries=q, max_distance=1.5)),
             ("radius_count", dict(queries=q, radius=2.0)), ("radius_count", dict(queries=q, radius=2.0, limit=3)),
             ("neighbour_distances", dict(k=8)), ("neighbour_distances", dict(k=1, max_distance=0.5)),
             ("orient_normals", dict(normals=normals, k=8, components=True)),
             ("orient_normals", dict(normals=normals, k=8, viewpoints=view)),
             ("smooth", dict(k=8, radius=2.0, curvature=True, order=True)),
             ("smooth", dict(k=8, radius=2.0, degree=1, normals=normals)),
             ("statistical_outliers", dict(k=8)), ("radius_outliers", dict(radius=2.0, min_neighbours=4)),
             ("cluster", dict(eps=1.0, min_points=3, core=True, stats=True)), ("cluster", dict(eps=0.5))]
    for k in (1, 8):
        calls.append(("knn", dict(queries=q, k=k)))
    calls.append(("knn", dict(queries=q, k=8, max_distance=2.0, indices=False)))
    for propagate in (False, True):
        calls.append(("estimate_normals", dict(k=8, variation=True, propagate=propagate)))
        calls.append(("estimate_normals", dict(k=8, viewpoints=view, propagate=propagate)))
    calls.append(("estimate_normals", dict(k=8, directions=normals)))
    for degree in (1, 2):
        calls.append(("project", dict(queries=q, k=8, radius=2.0, degree=degree, curvature=True, order=True)))
    assert len({name for name, _ in calls}) == 11
    for name, kw in calls:
        _same(getattr(f, name)(**kw), getattr(pi, name)(**kw), "%s(%s)" % (name, ", ".join(sorted(kw))))
    for kw in (dict(indices=True), dict(max_distance=2.0)):
        _same(f.distance_field(**kw), pi.distance_field(SIZES[D], **kw), "distance_field")


def _bad(name, *values):
    return [{name: v} for v in values]


NAN = math.nan
DISTANCE = _bad("max_distance", NAN, -1.0)
K = _bad("k", 0, 33)
MEMORY = _bad("memory", 7)
QUERIES = _bad("n", -1, 1 << 31) + _bad("queries", None)
# every way an operation's arguments can be wrong (the 32-bit limit of n: FI_ERR_UNSUPPORTED; the rest: FI_ERR_INVALID)
REFUSED = {
    "nearest": QUERIES + _bad("distances", None) + DISTANCE + MEMORY,
    "distance_field": _bad("out", None) + DISTANCE + MEMORY,
    "knn": QUERIES + _bad("distances", None) + K + DISTANCE + MEMORY,
    "estimate_normals": K + _bad("k", 1) + _bad("normals", None) + DISTANCE + MEMORY + _bad("orient", -1, 3),
    "orient_normals": K + _bad("normals", None) + DISTANCE + MEMORY + _bad("anchor", -1, 3),
    "mls_project": _bad("n", -1, 1 << 31) + K + _bad("radius", NAN, -1.0, 0.0, math.inf) + _bad("degree", 0, 3)
    + _bad("max_move", NAN, -1.0) + MEMORY + [dict(positions=None, normals=None, curvature=None, order=None)],
    "radius_count": QUERIES + _bad("counts", None) + _bad("radius", NAN, -1.0) + _bad("limit", 0) + MEMORY,
    "neighbour_distances": K + DISTANCE + MEMORY + [dict(mean=None, kth=None, counts=None)],
    "outliers_statistical": K + DISTANCE + _bad("std_ratio", NAN, -1.0) + MEMORY + [dict(keep=None, stats=None)],
    "outliers_radius": _bad("radius", NAN, -1.0) + _bad("min_neighbours", 0) + MEMORY + [dict(keep=None, num_kept=None)],
    "cluster": _bad("eps", NAN, -1.0, math.inf) + _bad("min_points", 0) + MEMORY + [dict(labels=None, stats=None)],
}
# the orientation argument of the two normals operations: guides missing, and their count against the set's 50 points
GUIDES = np.ones((50, 3), np.float32)
for _op, _mode in (("estimate_normals", "orient"), ("orient_normals", "anchor")):
    for _m in (1, 2):
        REFUSED[_op].append({_mode: _m, "guides": None, "num_guides": 50})
    REFUSED[_op] += [{_mode: _m, "guides": P.ptr(GUIDES), "num_guides": _n} for _m, _n in ((1, 2), (2, 1), (2, 49), (1, 0))]


def _code(changed):
    return 5 if changed.get("n") == 1 << 31 else 1


def test_refused_table_is_complete():
    assert sorted(REFUSED) == sorted(P.OPS)


@pytest.mark.parametrize("op", P.OPS)
def test_the_same_refusals_from_both_faces(fi, op):
    pos = np.random.default_rng(3).uniform(1, 8, size=(50, 3)).astype(np.float32)
    f = _field(fi, [10, 10, 10], pos)
    pi = fi.PointIndex(pos)
    b = P.Buffers(3, 50, 6, lattice=[10, 10, 10])             # (a context writes its own lattice's distance field)
    for changed in REFUSED[op]:
        of_context = P.call(P.CONTEXT_FACE, op, f._h, b, **changed)
        of_set = P.call(P.SET_FACE, op, pi._h, b, **changed)
        assert of_context == of_set and of_context[0] == _code(changed) and of_context[1], (changed, of_context, of_set)
    assert P.call(P.CONTEXT_FACE, op, f._h, b)[0] == 0 and P.call(P.SET_FACE, op, pi._h, b)[0] == 0


def test_the_order_of_a_context_s_refusals(fi):
    b = P.Buffers(3, 1, 4, lattice=[12, 10, 16])
    s = _field(fi, [12, 10, 16], np.array([[3.0, 4.0, 9.0]], np.float32), dtype="f32", rank=1, nranks=2)     # a slab context
    empty = _field(fi, [12, 10, 16])                                  # undivided, no points added
    for op in P.OPS:
        changed = REFUSED[op][0]
        assert P.call(P.CONTEXT_FACE, op, s._h, b, **changed)[0] == _code(changed) == 1, op    # the arguments first ...
        assert P.call(P.CONTEXT_FACE, op, s._h, b) == (5, SLAB_TEXT), op                        # ... then the slab ...
        if op in ("nearest", "knn", "radius_count", "mls_project"):
            assert P.call(P.CONTEXT_FACE, op, s._h, b, n=0) == (5, SLAB_TEXT), op               # ... also without a query
        if op in ("nearest", "knn", "radius_count"):
            assert P.call(P.CONTEXT_FACE, op, empty._h, b, n=0)[0] == 0, op
