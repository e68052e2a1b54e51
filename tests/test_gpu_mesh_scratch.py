"""The mesh units at the sizes where a packed scratch layout goes wrong.  Their temporaries are 256-byte aligned pieces of one
block (fi_arena.h), so a uint32[n + 1] piece of n = 63, 64 or 65 entries -- 256, 260, 264 bytes -- is followed directly by the
next piece: a write one entry too far lands in a neighbour instead of a buffer's slack.  Meshes of that many vertices and
primitives go through fi_mesh_parts / fi_mesh_measure / fi_mesh_select / fi_mesh_simplify, lattices whose count pass runs that
many work groups through both extractors, each against the numpy restatement of its contract as the unit's own test compares
them: tests/mesh_parts_reference.py (labels, integer columns, boxes and a selection's arrays equal, size and enclosed within
the restatement's own summation bound), tests/simplify_reference.py and tests/dual_reference.py (every array bit for bit),
tests/iso_reference.py (keys, indices, positions equal, normals within 1e-5).  The references are computed once."""
import functools

import numpy as np
import pytest

import dual_reference as DR
import iso_reference as R
import mesh_parts_reference as M
import simplify_reference as S

EDGE = (63, 64, 65)
PLACEMENTS = {"quadric": S.QUADRIC, "mean": S.MEAN}
CELL = 1.0


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- the meshes -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mesh_case(ndim, nv, npr):
    """nv vertices, npr primitives: a strip (2-D: a polyline) over the first vertices with a few chords across it, two loose
    primitives on vertices of their own, the last vertex unused; the primitives shuffled.  -> (vertices, normals, indices, the
    reference's Parts, {placement: the reference's simplification})"""
    rng = np.random.default_rng(1000 * ndim + 10 * nv + npr)
    used = nv - 1
    body = used - 2 * ndim                                      # the strip's vertices
    prims = [list(range(i, i + ndim)) if i % 2 == 0 or ndim == 2 else [i + 1, i, i + 2] for i in range(body - ndim + 1)]
    prims += [list(range(body + ndim * k, body + ndim * (k + 1))) for k in range(2)]
    extra = npr - len(prims)
    assert 0 < extra < 10
    prims += [[0, 2 * k + 2, 2 * k + 4][:ndim] for k in range(extra)]
    idx = np.array(prims, np.int32)[rng.permutation(npr)]
    assert idx.shape == (npr, ndim) and idx.max() == used - 1
    v = (rng.normal(size=(nv, ndim)) * 2.0).astype(np.float32)
    nrm = None
    if ndim == 3:
        nrm = rng.normal(size=(nv, 3))
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    simple = {name: S.simplify(v, nrm, idx, CELL, None, code) for name, code in PLACEMENTS.items()}
    return v, nrm, idx, M.Parts(v, idx), simple


MESHES = [(ndim, nv, npr) for ndim in (3, 2) for nv in EDGE for npr in EDGE]


@pytest.mark.parametrize("ndim,nv,npr", MESHES)
def test_reference_meshes_are_well_formed(ndim, nv, npr):
    v, _nrm, idx, parts, simple = mesh_case(ndim, nv, npr)
    assert len(v) == nv and len(idx) == npr
    assert parts.count >= 2 and (parts.vertex_labels == -1).sum() == 1 and parts.vertex_labels[-1] == -1
    assert parts.primitives.sum() == npr and parts.primitives.max() > nv // 2        # the strip and the loose ones
    for ref in simple.values():
        assert 0 < len(ref.indices) <= npr and 0 < len(ref.vertices) < nv and ref.vertex_map[-1] == -1


@pytest.mark.gpu
@pytest.mark.parametrize("ndim,nv,npr", MESHES)
def test_parts_measure_select(fi, ndim, nv, npr):
    v, nrm, idx, ref, _simple = mesh_case(ndim, nv, npr)
    mesh = fi.IsoMesh(v, nrm, idx, None)
    got = fi.mesh_parts(mesh)
    assert len(got.size) == ref.count
    assert np.array_equal(got.vertex_labels, ref.vertex_labels) and np.array_equal(got.primitive_labels, ref.primitive_labels)
    for name in ("vertices", "primitives", "edges", "boundary", "irregular", "closed", "euler"):
        assert np.array_equal(getattr(got, name), getattr(ref, name)), name
    assert np.array_equal(_bytes(got.lo), _bytes(ref.lo.astype(np.float32)))
    assert np.array_equal(_bytes(got.hi), _bytes(ref.hi.astype(np.float32)))
    # the two fp64 sums cannot be bit-equal to the restatement, which sums by math.fsum: they are held to its own bound for any
    # summation order, (P_c + 16) 2^-52 M_c, exactly as tests/test_gpu_mesh_parts.py holds them; every other array is exact
    assert (np.abs(got.size - ref.size) <= ref.size_bound).all()
    assert (np.abs(got.enclosed - ref.enclosed) <= ref.enclosed_bound).all()
    for part in (0, ref.count - 1):                             # the strip; a loose primitive
        keep = np.arange(ref.count) == part
        out = fi.select_parts(mesh, keep)
        want = M.select(v, nrm, idx, np.arange(nv, dtype=np.int64), ref.vertex_labels, ref.primitive_labels, keep)
        for a, b in zip(out, want):
            assert (a is None) == (b is None)
            assert a is None or (a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bytes(a), _bytes(b)))


@pytest.mark.gpu
@pytest.mark.parametrize("placement", sorted(PLACEMENTS))
@pytest.mark.parametrize("ndim,nv,npr", MESHES)
def test_simplify(fi, ndim, nv, npr, placement):
    v, nrm, idx, _parts, simple = mesh_case(ndim, nv, npr)
    ref = simple[placement]
    out, vmap = fi.simplify_mesh(fi.IsoMesh(v, nrm, idx, None), CELL, placement=placement, vertex_map=True)
    assert np.array_equal(vmap, ref.vertex_map) and vmap.dtype == np.int32
    assert np.array_equal(out.keys, ref.keys) and out.keys.dtype == np.int64
    assert out.indices.dtype == np.int32 and np.array_equal(out.indices, ref.indices)
    assert out.vertices.shape == ref.vertices.shape and np.array_equal(_bytes(out.vertices), _bytes(ref.vertices))
    assert (out.normals is None) == (ref.normals is None)
    if ref.normals is not None:
        assert np.array_equal(_bytes(out.normals), _bytes(ref.normals))


# ---- the lattices -----------------------------------------------------------------------------------------------------------

# a count pass runs one work group per 256 lattice points (fi_iso.hip) or cells (fi_dual.hip): 16128, 16384 and 16512 of them
# are 63, 64 and 64.5 groups
POINTS = {2: {63: [126, 128], 64: [128, 128], 65: [129, 128]}, 3: {63: [28, 24, 24], 64: [32, 32, 16], 65: [43, 24, 16]}}


@functools.lru_cache(maxsize=None)
def lattice_case(method, ndim, groups):
    """a random lattice whose count pass runs `groups` work groups -> (the field, the sizes, the reference's mesh)"""
    sizes = POINTS[ndim][groups] if method == "iso" else [n + 1 for n in POINTS[ndim][groups]]
    units = int(np.prod(sizes)) if method == "iso" else int(np.prod([n - 1 for n in sizes]))
    assert (units + 255) // 256 == groups
    f = np.random.default_rng(100 * ndim + groups).normal(size=int(np.prod(sizes))).astype(np.float32)
    return f, sizes, (R.extract(f, sizes, 0.0) if method == "iso" else DR.contour(f, sizes, 0.0, None)[:4])


LATTICES = [(method, ndim, groups) for method in ("iso", "dual") for ndim in (2, 3) for groups in EDGE]


@pytest.mark.parametrize("method,ndim,groups", LATTICES)
def test_reference_lattices_are_well_formed(method, ndim, groups):
    _f, _sizes, (v, n, idx, keys) = lattice_case(method, ndim, groups)
    assert len(v) > 256 and len(idx) > 256 and v.shape == n.shape == (len(keys), ndim) and idx.shape[1] == ndim
    assert np.all(np.diff(keys) > 0) and idx.min() >= 0 and idx.max() < len(v)


@pytest.mark.gpu
@pytest.mark.parametrize("method,ndim,groups", LATTICES)
def test_extractors(fi, method, ndim, groups):
    f, sizes, (v, n, idx, keys) = lattice_case(method, ndim, groups)
    mesh = (fi.iso_surface if method == "iso" else fi.dual_contour)(f, sizes, 0.0)
    assert np.array_equal(mesh.keys, keys) and np.array_equal(mesh.indices, idx)
    assert mesh.vertices.shape == v.shape and np.array_equal(_bytes(mesh.vertices), _bytes(v))
    if method == "iso":
        assert np.abs(mesh.normals - n).max() <= 1e-5
    else:
        assert np.array_equal(_bytes(mesh.normals), _bytes(n))
