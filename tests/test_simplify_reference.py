"""The numpy restatement of the mesh-simplification contract (tests/simplify_reference.py; include/fi_hip.h fi_mesh_simplify,
DESIGN.md 4.15) held to answers known without it: the exactly tessellated cube whose corners and volume the quadric placement
must restore, the sphere whose deviation it must lower, the identity and the weld at a cell below the vertex spacing, small
constructed meshes, and its vectorised sums against a plain loop.  No GPU."""
import numpy as np
import pytest

import iso_reference as R
import mesh_parts_reference as M
import simplify_reference as S


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def sphere():
    f, centre = S.sphere_field()
    return R.extract(f, [24, 24, 24]) + (np.asarray(centre),)


# ---- the exact cube -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", [2.0, 2.5])
def test_cube_corners_and_volume(cell):
    v, t = S.cube_mesh(12, 2.25, 0.75)
    assert (len(v), len(t)) == (866, 1728) and R.watertight_oriented(t)
    lo, hi = 2.25, 11.25
    q = S.simplify(v, None, t, cell, None, S.QUADRIC)
    m = S.simplify(v, None, t, cell, None, S.MEAN)
    for r in (q, m):
        assert (len(r.vertices), len(r.indices)) == (98, 192) and R.watertight_oriented(r.indices)
        assert r.normals is None and np.all(np.diff(r.keys) > 0)
    assert q.fallbacks == 0
    # every vertex on the surface, eight of them at the corners: within 4 fp32 ulps of the coordinate 11.25 (the restatement
    # gives 0: the faces' planes are exact in fp64 and the corner is their only common point)
    tol = 4 * np.spacing(np.float32(hi))
    x = q.vertices.astype(np.float64)
    off = np.minimum(np.abs(x - lo), np.abs(x - hi)).min(axis=1)
    inside = np.all((x >= lo - tol) & (x <= hi + tol), axis=1)
    print("cube cell %g: largest distance from the surface %.3g" % (cell, off.max()))
    assert inside.all() and off.max() <= tol
    corners = np.array([[a, b, c] for a in (lo, hi) for b in (lo, hi) for c in (lo, hi)])
    d = np.abs(x[None, :, :] - corners[:, None, :]).max(axis=2).min(axis=1)
    print("cube cell %g: largest corner miss, quadric %.3g" % (cell, d.max()))
    assert d.max() <= tol
    dm = np.abs(m.vertices.astype(np.float64)[None, :, :] - corners[:, None, :]).max(axis=2).min(axis=1)
    assert dm.max() > 1000 * tol                                # the mean rounds corners off
    vq, vm = R.signed_measure(q.vertices, q.indices), R.signed_measure(m.vertices, m.indices)
    print("cube cell %g: volume quadric %.9g mean %.9g" % (cell, vq, vm))
    assert abs(vq - 729.0) < abs(vm - 729.0) / 100


# ---- the sphere ---------------------------------------------------------------------------------------------------------

def _deviation(r, centre, radius=9.0):
    x = r.vertices.astype(np.float64)
    cen = x[r.indices].mean(axis=1)
    return max(np.abs(np.linalg.norm(x - centre, axis=1) - radius).max(), np.abs(np.linalg.norm(cen - centre, axis=1) - radius).max())


@pytest.mark.parametrize("cell", [2, 3, 4])
def test_sphere_stays_closed_and_quadric_is_closer(sphere, cell):
    pos, nrm, idx, _keys, centre = sphere
    assert (len(pos), len(idx)) == (1528, 3052)
    q = S.simplify(pos, nrm, idx, cell, None, S.QUADRIC)
    m = S.simplify(pos, nrm, idx, cell, None, S.MEAN)
    for r in (q, m):
        assert R.watertight_oriented(r.indices) and R.euler_characteristic(len(r.vertices), r.indices) == 2
        assert len(r.indices) < len(idx) / 3 and np.array_equal(r.indices, q.indices)
        n = np.linalg.norm(r.normals.astype(np.float64), axis=1)
        assert np.abs(n - 1).max() < 1e-6
    assert q.fallbacks == 0
    dq, dm = _deviation(q, centre), _deviation(m, centre)
    print("sphere cell %g: %d triangles, deviation quadric %.3f mean %.3f" % (cell, len(q.indices), dq, dm))
    assert dq < dm


# ---- identity and weld --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("placement", [S.QUADRIC, S.MEAN])
def test_identity_below_the_vertex_spacing(sphere, placement):
    pos, nrm, idx, _keys, _c = sphere
    r = S.simplify(pos, nrm, idx, 1e-3, None, placement)
    assert r.clusters == len(pos) and len(r.vertices) == len(pos) and r.fallbacks == 0
    assert np.array_equal(_bits(r.vertices[r.vertex_map]), _bits(pos))
    # (a normal that is unit in fp32 is not quite so in fp64: dividing by its length again may move the last bit)
    assert np.abs(r.normals[r.vertex_map] - nrm).max() <= 2.0 ** -23
    assert np.array_equal(r.vertex_map[idx], r.indices)                    # the primitives, renumbered
    assert np.array_equal(np.sort(r.vertex_map), np.arange(len(pos)))


def test_weld_of_a_soup():
    pos, _nrm, idx, _keys = R.extract(M.fixture_3d(), M.FIXTURE_3D_SIZES)
    parts = M.Parts(pos, idx)
    keep = np.arange(parts.count) == 1                                        # the closed sphere of the fixture
    pos, _n, idx, _k = M.select(pos, None, idx, np.arange(len(pos)), parts.vertex_labels, parts.primitive_labels, keep)
    sv, si, _ = S.soup(pos, idx)
    assert len(sv) == 3 * len(idx) and M.labels(len(sv), si)[0] == len(idx)   # one part per triangle
    r = S.simplify(sv, None, si, 1e-3, None, S.MEAN)
    assert len(r.vertices) == len(pos) and len(r.indices) == len(idx) and R.watertight_oriented(r.indices)
    # the indexed positions bit for bit: a welded vertex is the mean of equal values
    order = np.lexsort(pos.T[::-1])
    got = np.lexsort(r.vertices.T[::-1])
    assert np.array_equal(_bits(r.vertices[got]), _bits(pos[order]))
    assert M.labels(len(r.vertices), r.indices)[0] == 1


# ---- constructed cases --------------------------------------------------------------------------------------------------

def test_duplicates_reverses_degenerates_and_unused():
    # clusters at cell 1: vertices 0,1 -> cell (0,0,0); 2 -> (3,0,0); 3 -> (0,3,0); 4 unused; 5 -> (0,0,3)
    v = np.array([[0.2, 0.2, 0.2], [0.6, 0.4, 0.3], [3.5, 0.5, 0.5], [0.5, 3.5, 0.5], [9.5, 9.5, 9.5], [0.5, 0.5, 3.5]], np.float32)
    t = np.array([[0, 2, 3],        # kept
                  [2, 3, 1],        # the same oriented triple through vertex 1, rotated: dropped
                  [3, 2, 0],        # the reverse: kept
                  [0, 1, 2],        # two vertices in one cluster: dropped
                  [5, 5, 2],        # a repeated index: dropped
                  [0, 3, 5]], np.int32)
    r = S.simplify(v, None, t, 1.0, None, S.MEAN)
    assert r.clusters == 4 and len(r.vertices) == 4
    assert r.vertex_map.tolist() == [0, 0, 1, 2, -1, 3]
    assert r.indices.tolist() == [[0, 1, 2], [2, 1, 0], [0, 2, 3]]
    assert np.array_equal(_bits(r.vertices[0]), _bits(((v[0].astype(np.float64) - 0.5) + (v[1].astype(np.float64) - 0.5)) / 2 + 0.5))
    # a cluster no survivor uses does not come out: only [5, 5, 2] and a degenerate use vertex 5 here
    r2 = S.simplify(v, None, t[:5], 1.0, None, S.QUADRIC)
    assert r2.clusters == 4 and len(r2.vertices) == 3 and r2.vertex_map.tolist() == [0, 0, 1, 2, -1, -1]
    # everything in one cell
    r3 = S.simplify(v, None, t, 64.0, None, S.QUADRIC)
    assert len(r3.vertices) == 0 and r3.indices.shape == (0, 3) and (r3.vertex_map == -1).all() and r3.clusters == 1
    # no primitives, no vertices
    r4 = S.simplify(v, v, np.zeros((0, 3), np.int32), 1.0)
    assert len(r4.vertices) == 0 and r4.normals.shape == (0, 3) and (r4.vertex_map == -1).all()


def _grid_patch(f, n=9, h=0.25):
    """the graph z = f(x, y) over an n x n grid of spacing h, two triangles a quad"""
    x, y = np.meshgrid(np.arange(n) * h, np.arange(n) * h, indexing="xy")
    v = np.stack([x, y, f(x, y)], axis=2).reshape(-1, 3).astype(np.float32)
    i = (np.arange(n - 1)[None, :] + n * np.arange(n - 1)[:, None]).reshape(-1)
    t = np.concatenate([np.stack([i, i + 1, i + n + 1], axis=1), np.stack([i, i + n + 1, i + n], axis=1)])
    return v, t.astype(np.int32)


def test_rank_deficient_quadrics():
    # rank 1, a plane: the minimiser moves the mean along the normal only, i.e. not at all
    v, t = _grid_patch(lambda x, y: 0.5 + 0 * x)
    q, m = S.simplify(v, None, t, 1.0), S.simplify(v, None, t, 1.0, None, S.MEAN)
    assert q.fallbacks == 0 and len(q.vertices) == 9
    assert np.abs(q.vertices.astype(np.float64) - m.vertices).max() < 1e-6 and np.all(q.vertices[:, 2] == 0.5)
    # rank 2, a crease along y at x = 1: the clusters it crosses land on it, and keep the mean's y
    v, t = _grid_patch(lambda x, y: 0.25 + np.abs(x - 1.0) * 0.5)
    q, m = S.simplify(v, None, t, 0.75, [0.1, 0.0, 0.0]), S.simplify(v, None, t, 0.75, [0.1, 0.0, 0.0], S.MEAN)
    assert q.fallbacks == 0
    on = np.abs(m.vertices[:, 0] - 1.0) < 0.3                     # the clusters that hold both sides
    assert on.sum() == 3
    assert np.abs(q.vertices[on, 0] - 1.0).max() < 1e-6 and np.abs(q.vertices[on, 2] - 0.25).max() < 1e-6
    assert np.abs(q.vertices[on, 1] - m.vertices[on, 1]).max() < 1e-6
    assert np.abs(m.vertices[on, 2] - 0.25).min() > 0.05          # the mean floats above the crease
    # a cluster that sees zero-area triangles only (its three vertices on a line with the others' clusters): A = 0, the mean
    v = np.array([[0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [2.5, 0.5, 0.5], [4.5, 0.5, 0.5]], np.float32)
    t = np.array([[0, 2, 3], [1, 3, 2]], np.int32)
    q, m = S.simplify(v, None, t, 1.0), S.simplify(v, None, t, 1.0, None, S.MEAN)
    assert q.fallbacks == 0 and q.indices.tolist() == [[0, 1, 2], [0, 2, 1]]
    assert np.array_equal(_bits(q.vertices), _bits(m.vertices)) and q.vertices[0].tolist() == [0.5, 0.5, 0.5]


def test_negative_coordinates_and_origin():
    v = np.array([[-0.25, -0.25, 0.0], [-0.75, -0.5, 0.0], [-1.25, 0.5, 0.0], [0.5, -1.5, 0.0], [0.25, 0.25, 0.0]], np.float32)
    t = np.array([[0, 2, 3], [1, 2, 3], [4, 2, 3]], np.int32)
    r = S.simplify(v, None, t, 1.0, None, S.MEAN)
    # floor, not truncation: -0.25 and -0.75 share cell -1, 0.25 does not
    assert r.vertex_map[0] == r.vertex_map[1] != r.vertex_map[4] and len(r.indices) == 2
    cells = [[(k >> (21 * a) & 0x1FFFFF) - S.BIAS for a in range(3)] for k in r.keys.tolist()]
    assert sorted(cells) == sorted([[-1, -1, 0], [-2, 0, 0], [0, -2, 0], [0, 0, 0]])
    # a shifted origin moves the walls: with o = (-0.5, -0.5, 0) vertex 0 joins vertex 4 and leaves vertex 1
    s = S.simplify(v, None, t, 1.0, [-0.5, -0.5, 0.0], S.MEAN)
    assert s.vertex_map[0] == s.vertex_map[4] != s.vertex_map[1]
    with pytest.raises(S.Invalid):
        S.simplify(v, None, t, 1e-7)                                # 0.25 / 1e-7 cells from the origin
    with pytest.raises(S.Invalid):
        S.simplify(np.where(np.arange(15).reshape(5, 3) == 7, np.nan, v), None, t, 1.0)
    S.simplify(np.concatenate([v, [[np.nan] * 3]]).astype(np.float32), None, t, 1.0)   # an unused vertex may be anything
    for bad in (0.0, -1.0, np.nan):
        with pytest.raises(S.Invalid):
            S.simplify(v, None, t, bad)
    with pytest.raises(S.Invalid):
        S.simplify(v, None, t, 1.0, None, 2)


def test_square_polyline_corners_exact():
    v, s = S.square_polyline(8, 1.5, 0.5)
    assert R.watertight_oriented(s)
    q, m = S.simplify(v, None, s, 1.5, None, S.QUADRIC), S.simplify(v, None, s, 1.5, None, S.MEAN)
    assert q.indices.shape[1] == 2 and R.watertight_oriented(q.indices) and q.fallbacks == 0
    corners = {(1.5, 1.5), (5.5, 1.5), (5.5, 5.5), (1.5, 5.5)}
    assert corners <= {tuple(p) for p in q.vertices.tolist()}
    assert not corners & {tuple(p) for p in m.vertices.tolist()}
    assert R.signed_measure(q.vertices, q.indices) == 16.0 and R.signed_measure(m.vertices, m.indices) < 15.9


# ---- the vectorised sums ------------------------------------------------------------------------------------------------

def test_vectorised_sums_are_the_serial_ones(sphere):
    """np.add.at adds one entry after the other: the same bytes as a Python loop in ascending order"""
    pos, nrm, idx, _keys, _c = sphere
    cell, o = np.float32(2.0), np.zeros(3, np.float32)
    idx = idx.astype(np.int64)
    cells, keys = S.cell_keys(pos, cell, o)
    ckeys, first, cluster_of = np.unique(keys, return_index=True, return_inverse=True)
    K = len(ckeys)
    g = (cells[first].astype(np.float64) + 0.5) * np.float64(cell)
    pos64 = pos.astype(np.float64)
    rel = pos64 - g[cluster_of]
    s, cnt, ns = S.cluster_sums(rel, nrm.astype(np.float64), np.arange(len(pos)), cluster_of, K)
    s2, ns2 = np.zeros_like(s), np.zeros_like(ns)
    for v in range(len(pos)):
        for d in range(3):
            s2[cluster_of[v], d] = s2[cluster_of[v], d] + rel[v, d]
            ns2[cluster_of[v], d] = ns2[cluster_of[v], d] + np.float64(nrm[v, d])
    assert np.array_equal(s.view(np.uint64), s2.view(np.uint64)) and np.array_equal(ns.view(np.uint64), ns2.view(np.uint64))
    assert np.array_equal(cnt, np.bincount(cluster_of))
    cl, At, bt = S.primitive_terms(idx, pos64, cluster_of, g)
    A, b = np.zeros((K, 3, 3)), np.zeros((K, 3))
    np.add.at(A, cl, At)
    np.add.at(b, cl, bt)
    A2, b2 = np.zeros((K, 3, 3)), np.zeros((K, 3))
    for p in range(len(idx)):
        seen = []
        for k in range(3):
            c = cluster_of[idx[p, k]]
            if c in seen:
                continue
            seen.append(c)
            a_, b_, c_ = (pos64[idx[p, j]] - g[c] for j in range(3))
            u, w = b_ - a_, c_ - a_
            n = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
            na = (n[0] * a_[0] + n[1] * a_[1]) + n[2] * a_[2]
            for i in range(3):
                b2[c, i] = b2[c, i] + n[i] * na
                for j in range(3):
                    A2[c, i, j] = A2[c, i, j] + n[i] * n[j]
    assert np.array_equal(A.view(np.uint64), A2.view(np.uint64)) and np.array_equal(b.view(np.uint64), b2.view(np.uint64))
