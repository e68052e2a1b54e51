"""The numpy restatement of the mesh-parts contract (tests/mesh_parts_reference.py) against answers known beforehand: exact
solids and loops, and the three fields the GPU tests use, extracted by tests/iso_reference.py."""
import math

import numpy as np
import pytest

import iso_reference as R
import mesh_parts_reference as M

TETRA = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32),
         np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32))
CUBE = (np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32),
        np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2],
                  [1, 3, 7], [1, 7, 5]], np.int32))
OCTA = (np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32),
        np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32))


@pytest.mark.parametrize("solid, volume, area, nv, ne, nf", [
    (TETRA, 1.0 / 6.0, 1.5 + math.sqrt(3.0) / 2.0, 4, 6, 4),
    (CUBE, 1.0, 6.0, 8, 18, 12),
    (OCTA, 4.0 / 3.0, 4.0 * math.sqrt(3.0), 6, 12, 8)], ids=["tetrahedron", "cube", "octahedron"])
def test_exact_solids(solid, volume, area, nv, ne, nf):
    v, idx = solid
    p = M.Parts(v, idx)
    assert p.count == 1 and (p.vertex_labels == 0).all() and (p.primitive_labels == 0).all()
    assert (p.vertices[0], p.edges[0], p.primitives[0], p.boundary[0], p.irregular[0]) == (nv, ne, nf, 0, 0)
    assert p.closed[0] and p.euler[0] == 2
    assert abs(p.enclosed[0] - volume) <= 1e-15 and abs(p.size[0] - area) <= 1e-14
    assert np.array_equal(p.lo[0], v.min(axis=0)) and np.array_equal(p.hi[0], v.max(axis=0))
    # turned inside out: the same counts, the volume negated; moved: the same volume (the part is closed)
    q = M.Parts(v + np.float32(3.0), idx[:, ::-1])
    assert q.closed[0] and q.euler[0] == 2 and abs(q.enclosed[0] + volume) <= 1e-13


def test_exact_loops():
    v = np.array([[0, 0], [2, 0], [2, 2], [0, 2], [5, 5], [6, 5], [5, 6], [9, 9]], np.float32)
    idx = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [4, 6], [6, 5], [5, 4]], np.int32)
    p = M.Parts(v, idx)
    assert p.count == 2
    assert list(p.vertex_labels) == [0, 0, 0, 0, 1, 1, 1, -1] and list(p.primitive_labels) == [0, 0, 0, 0, 1, 1, 1]
    assert list(p.vertices) == [4, 3] and list(p.edges) == [4, 3] and list(p.boundary) == [0, 0] and list(p.irregular) == [0, 0]
    assert p.closed.all() and list(p.euler) == [0, 0]
    assert p.size[0] == 8.0 and p.enclosed[0] == 4.0                      # counter-clockwise: a blob
    assert abs(p.size[1] - (2.0 + math.sqrt(2.0))) <= 1e-15 and p.enclosed[1] == -0.5   # clockwise: a cavity
    assert np.array_equal(p.lo, [[0, 0], [5, 5]]) and np.array_equal(p.hi, [[2, 2], [6, 6]])


def test_irregular_and_degenerate():
    v = np.zeros((6, 3), np.float32)
    # two triangles running the same way along the edge (0, 1); a triangle with a repeated index; an unused vertex
    p = M.Parts(v, np.array([[0, 1, 2], [0, 1, 3], [4, 4, 3]], np.int32))
    assert p.count == 1 and p.vertex_labels[5] == -1
    assert (p.vertices[0], p.primitives[0], p.edges[0], p.boundary[0], p.irregular[0]) == (5, 3, 6, 4, 1)
    # 2-D: a fork (vertex 1 has three segments), and a segment of equal ends
    q = M.Parts(np.zeros((5, 2), np.float32), np.array([[0, 1], [1, 2], [1, 3], [4, 4]], np.int32))
    assert q.count == 2 and list(q.edges) == [3, 0] and list(q.boundary) == [3, 0] and list(q.irregular) == [1, 1]


def test_select_restatement():
    v = np.arange(14, dtype=np.float32).reshape(7, 2)
    idx = np.array([[5, 6], [0, 1], [3, 4], [1, 0]], np.int32)
    keys = np.arange(7, dtype=np.int64) * 10
    C, vl, pl = M.labels(7, idx)
    assert C == 3 and list(vl) == [0, 0, -1, 1, 1, 2, 2] and list(pl) == [2, 0, 1, 0]
    sv, sn, si, sk = M.select(v, None, idx, keys, vl, pl, [True, False, True])
    assert sn is None and list(sk) == [0, 10, 50, 60] and si.tolist() == [[2, 3], [0, 1], [1, 0]]
    assert np.array_equal(sv, v[[0, 1, 5, 6]])
    assert len(M.select(v, None, idx, keys, vl, pl, [False] * 3)[2]) == 0


@pytest.fixture(scope="module")
def mesh3():
    return R.extract(M.fixture_3d(), M.FIXTURE_3D_SIZES)


def test_fixture_3d(mesh3):
    v, _n, idx, _k = mesh3
    assert (len(v), len(idx)) == (1070, 2088)
    p = M.Parts(v, idx)
    assert p.count == 4
    assert list(zip(p.vertices, p.primitives, p.edges)) == [(148, 252, 399), (310, 616, 924), (512, 1024, 1536), (100, 196, 294)]
    assert list(p.boundary) == [42, 0, 0, 0] and list(p.irregular) == [0, 0, 0, 0]
    assert list(p.euler) == [1, 2, 0, 2] and list(p.closed) == [False, True, True, True]
    assert np.allclose(p.enclosed[1:], [278.44, 308.89, 45.245], rtol=0, atol=[0.005, 0.005, 0.0005])   # (to the digits stated)
    # the large sphere: 3.6 % below 4/3 pi r^3 (the triangles are chords of it)
    assert abs(p.enclosed[1] / (4.0 / 3.0 * math.pi * 4.1 ** 3) - (1 - 0.036)) < 0.001
    assert int(np.argmax(p.size)) == 2 and abs(p.size[2] - 339.2) < 0.05          # the torus has the largest area


def test_fixture_3d_negated(mesh3):
    p = M.Parts(mesh3[0], mesh3[2])
    v, _n, idx, _k = R.extract(-M.fixture_3d(), M.FIXTURE_3D_SIZES)
    q = M.Parts(v, idx)
    for name in ("vertices", "primitives", "edges", "boundary", "irregular"):
        assert np.array_equal(getattr(p, name), getattr(q, name)), name
    assert np.allclose(q.enclosed[1:], -p.enclosed[1:], rtol=1e-9)


def test_fixture_2d():
    v, _n, idx, _k = R.extract(M.fixture_2d(), M.FIXTURE_2D_SIZES)
    assert (len(v), len(idx)) == (113, 112)
    p = M.Parts(v, idx)
    assert p.count == 4
    assert list(p.boundary) == [2, 0, 0, 0] and list(p.irregular) == [0, 0, 0, 0] and list(p.closed) == [False, True, True, True]
    assert (p.vertices - p.edges).tolist() == [1, 0, 0, 0] and np.array_equal(p.edges, p.primitives)
    assert np.allclose(p.enclosed[1:], [116.24, -17.44, 31.52], rtol=0, atol=0.005)   # (to the digits stated)
    for c, exact in ((1, math.pi * 6.1 ** 2), (2, -math.pi * 2.4 ** 2), (3, math.pi * 3.2 ** 2)):
        assert abs(p.enclosed[c] - exact) <= 0.05 * abs(exact)
    assert abs(p.enclosed[3] / (math.pi * 3.2 ** 2) - 0.98) < 0.001


def test_checkerboard():
    v, _n, idx, _k = R.extract(M.checkerboard(), M.CHECKERBOARD_SIZES)
    C, vl, _pl = M.labels(len(v), idx)
    assert (len(v), len(idx), C) == (1321, 1344, 252) and (vl >= 0).all()


def test_labels_of_a_long_permuted_chain():
    n = 5000
    perm = np.random.default_rng(5).permutation(n + 1)
    idx = np.stack([perm[:-1], perm[1:]], axis=1).astype(np.int32)
    for chain in (idx, idx[::-1, ::-1]):
        C, vl, pl = M.labels(n + 1, chain)
        assert C == 1 and (vl == 0).all() and (pl == 0).all()
        c = M.counts(n + 1, chain, vl, pl, C)
        assert (c["vertices"][0], c["edges"][0], c["boundary"][0], c["irregular"][0]) == (n + 1, n, 2, 0)


@pytest.mark.parametrize("ndim", [2, 3])
def test_empty_meshes(ndim):
    # no vertices at all (what an extractor returns where nothing crosses iso), and vertices that no primitive uses
    p = M.Parts(np.empty((0, ndim), np.float32), np.empty((0, ndim), np.int32))
    assert p.count == 0 and len(p.vertex_labels) == 0 and len(p.primitive_labels) == 0 and len(p.size) == 0 and len(p.edges) == 0
    q = M.Parts(np.ones((3, ndim), np.float32), np.empty((0, ndim), np.int32))
    assert q.count == 0 and list(q.vertex_labels) == [-1, -1, -1] and q.lo.shape == (0, ndim)
    out = M.select(np.ones((3, ndim), np.float32), None, np.empty((0, ndim), np.int32), np.arange(3), q.vertex_labels,
                   q.primitive_labels, [])
    assert out[0].shape == (0, ndim) and out[2].shape == (0, ndim) and len(out[3]) == 0
