"""Mesh simplification on the device (fi_simplify.hip through fi_mesh_simplify, simplify_mesh and the extractors' simplify
keyword) against the numpy restatement of the contract (tests/simplify_reference.py): every output array -- positions, normals,
indices, keys, the vertex map -- bit for bit, plus the invariants that hold for every result."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import iso_reference as R
import mesh_parts_reference as M
import simplify_reference as S

pytestmark = pytest.mark.gpu

ORIGINS = (None, (-0.37, 0.21, 0.5))
PLACEMENTS = ("quadric", "mean")


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_mesh(a, b):
    for u, w in zip(a, b):
        assert (u is None) == (w is None)
        if u is not None:
            assert u.dtype == w.dtype and u.shape == w.shape and np.array_equal(_bytes(u), _bytes(w))


def _invariants(mesh, out, vmap, cell, what):
    nv, D = out.vertices.shape
    idx = out.indices.astype(np.int64)
    assert out.indices.dtype == np.int32 and idx.shape[1] == D, what
    if len(idx):
        assert idx.min() >= 0 and idx.max() < nv, what
        assert np.all(idx[:, 0] != idx[:, 1]), what
        if D == 3:
            assert np.all(idx[:, 1] != idx[:, 2]) and np.all(idx[:, 0] != idx[:, 2]), what
        assert len(np.unique(S.canonical(idx), axis=0)) == len(idx), what          # no oriented tuple twice
    used = np.zeros(nv, bool)
    used[idx.reshape(-1)] = True
    assert used.all(), what
    assert np.all(np.diff(out.keys) > 0), what
    on = vmap >= 0
    assert vmap.dtype == np.int32 and vmap.shape == (len(mesh.vertices),) and (vmap[on] < nv).all(), what
    if on.any():
        p = np.asarray(mesh.vertices, np.float32)[on].astype(np.float64)
        moved = np.abs(p - out.vertices[vmap[on]].astype(np.float64)).max()
        slack = 4 * float(np.spacing(np.float32(np.abs(p).max() + 2 * cell)))
        assert moved <= 1.5 * float(np.float32(cell)) + slack, (what, moved)


def _check(fi, mesh, cell, origin=None, placement="quadric", what=""):
    """simplify_mesh of an IsoMesh of numpy arrays against the restatement -> (the device's mesh, its vertex map, the Result)"""
    what = "%s cell %g origin %s %s" % (what, cell, origin, placement)
    D = mesh.vertices.shape[1]
    o = None if origin is None else origin[:D]
    ref = S.simplify(mesh.vertices, mesh.normals, mesh.indices, cell, o, S.QUADRIC if placement == "quadric" else S.MEAN)
    out, vmap = fi.simplify_mesh(mesh, cell, origin=o, placement=placement, vertex_map=True)
    assert out.vertices.shape == ref.vertices.shape and out.indices.shape == ref.indices.shape, (what, out.vertices.shape, ref.vertices.shape)
    assert np.array_equal(out.keys, ref.keys) and out.keys.dtype == np.int64, what
    assert np.array_equal(vmap, ref.vertex_map), what
    assert np.array_equal(out.indices, ref.indices), what
    diff = np.flatnonzero((out.vertices.view(np.uint32) != ref.vertices.view(np.uint32)).any(axis=1))
    assert len(diff) == 0, (what, len(diff), out.vertices[diff[:3]], ref.vertices[diff[:3]])
    assert (out.normals is None) == (ref.normals is None), what
    if ref.normals is not None:
        assert np.array_equal(out.normals.view(np.uint32), ref.normals.view(np.uint32)), what
    _invariants(mesh, out, vmap, cell, what)
    return out, vmap, ref


def _mesh(fi, v, idx, normals=None, keys=None):
    return fi.IsoMesh(np.asarray(v, np.float32), normals, np.asarray(idx, np.int32), keys)


@pytest.fixture(scope="module")
def sphere(fi):
    f, centre = S.sphere_field()
    return fi.IsoMesh(*R.extract(f, [24, 24, 24])), np.asarray(centre)


# ---- the cases of tests/test_simplify_reference.py ------------------------------------------------------------------------

@pytest.mark.parametrize("placement", PLACEMENTS)
def test_cube(fi, placement):
    v, t = S.cube_mesh(12, 2.25, 0.75)
    for cell in (2.0, 2.5):
        out, _vm, _ref = _check(fi, _mesh(fi, v, t), cell, None, placement, "cube")
        assert (len(out.vertices), len(out.indices)) == (98, 192) and out.normals is None


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_sphere(fi, sphere, placement):
    mesh, _c = sphere
    for cell in (2, 3, 4):
        out, _vm, ref = _check(fi, mesh, cell, None, placement, "sphere")
        assert ref.fallbacks == 0 and R.watertight_oriented(out.indices)
    out, vmap, _ref = _check(fi, mesh, 1e-3, None, placement, "identity")
    assert np.array_equal(out.vertices[vmap].view(np.uint32), mesh.vertices.view(np.uint32))
    assert np.array_equal(vmap[mesh.indices], out.indices)


def test_weld(fi):
    pos, nrm, idx, _keys = R.extract(M.fixture_3d(), M.FIXTURE_3D_SIZES)
    sv, si, sn = S.soup(pos, idx, nrm)
    soup = _mesh(fi, sv, si, sn)
    assert len(fi.mesh_parts(soup).size) == len(idx)            # a part per triangle before ...
    out, _vm, _ref = _check(fi, soup, 1e-3, None, "mean", "weld")
    assert len(out.vertices) == len(pos) and len(out.indices) == len(idx)
    assert len(fi.mesh_parts(out).size) == 4                    # ... and the fixture's four after
    _check(fi, soup, 1e-3, None, "quadric", "weld")


def test_constructed_cases(fi):
    v = np.array([[0.2, 0.2, 0.2], [0.6, 0.4, 0.3], [3.5, 0.5, 0.5], [0.5, 3.5, 0.5], [9.5, 9.5, 9.5], [0.5, 0.5, 3.5]], np.float32)
    t = np.array([[0, 2, 3], [2, 3, 1], [3, 2, 0], [0, 1, 2], [5, 5, 2], [0, 3, 5]], np.int32)
    n = np.random.default_rng(5).normal(size=v.shape).astype(np.float32)
    n[:2] = [[1, 0, 0], [-1, 0, 0]]                               # cluster 0's normals cancel: zeros
    for placement in PLACEMENTS:
        out, vmap, _r = _check(fi, _mesh(fi, v, t, n), 1.0, None, placement, "duplicates")
        assert out.indices.tolist() == [[0, 1, 2], [2, 1, 0], [0, 2, 3]] and vmap.tolist() == [0, 0, 1, 2, -1, 3]
        assert out.normals[0].tolist() == [0, 0, 0]
        out, vmap, _r = _check(fi, _mesh(fi, v, t[:5]), 1.0, None, placement, "a cluster nothing uses")
        assert len(out.vertices) == 3 and vmap.tolist() == [0, 0, 1, 2, -1, -1]
        out, vmap, _r = _check(fi, _mesh(fi, v, t, n), 64.0, None, placement, "one cell")
        assert out.vertices.shape == (0, 3) and out.indices.shape == (0, 3) and out.normals.shape == (0, 3) and (vmap == -1).all()
    # no primitives; nothing at all
    out, vmap = fi.simplify_mesh(_mesh(fi, v, np.zeros((0, 3), np.int32)), 1.0, vertex_map=True)
    assert len(out.vertices) == 0 and len(out.indices) == 0 and (vmap == -1).all() and len(vmap) == 6
    out, vmap = fi.simplify_mesh(_mesh(fi, np.zeros((0, 2)), np.zeros((0, 2), np.int32)), 1.0, vertex_map=True)
    assert out.vertices.shape == (0, 2) and len(vmap) == 0
    # an unused vertex may be anything
    _check(fi, _mesh(fi, np.concatenate([v, [[np.nan, np.inf, 0]]]), t), 1.0, None, "quadric", "unused NaN")


def _grid_patch(f, n=9, h=0.25):
    x, y = np.meshgrid(np.arange(n) * h, np.arange(n) * h, indexing="xy")
    v = np.stack([x, y, f(x, y)], axis=2).reshape(-1, 3).astype(np.float32)
    i = (np.arange(n - 1)[None, :] + n * np.arange(n - 1)[:, None]).reshape(-1)
    t = np.concatenate([np.stack([i, i + 1, i + n + 1], axis=1), np.stack([i, i + n + 1, i + n], axis=1)])
    return v, t.astype(np.int32)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_rank_deficient_and_signs(fi, placement):
    _check(fi, _mesh(fi, *_grid_patch(lambda x, y: 0.5 + 0 * x)), 1.0, None, placement, "plane")
    _check(fi, _mesh(fi, *_grid_patch(lambda x, y: 0.25 + np.abs(x - 1.0) * 0.5)), 0.75, (0.1, 0.0, 0.0), placement, "crease")
    v = np.array([[0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [2.5, 0.5, 0.5], [4.5, 0.5, 0.5]], np.float32)
    _check(fi, _mesh(fi, v, [[0, 2, 3], [1, 3, 2]]), 1.0, None, placement, "zero areas")
    v = np.array([[-0.25, -0.25, 0.0], [-0.75, -0.5, 0.0], [-1.25, 0.5, 0.0], [0.5, -1.5, 0.0], [0.25, 0.25, 0.0]], np.float32)
    t = [[0, 2, 3], [1, 2, 3], [4, 2, 3]]
    _out, vmap, _r = _check(fi, _mesh(fi, v, t), 1.0, None, placement, "negative")
    assert vmap[0] == vmap[1] != vmap[4]
    _out, vmap, _r = _check(fi, _mesh(fi, v, t), 1.0, (-0.5, -0.5, 0.0), placement, "shifted origin")
    assert vmap[0] == vmap[4] != vmap[1]
    sv, ss = S.square_polyline(8, 1.5, 0.5)
    out, _vm, _r = _check(fi, _mesh(fi, sv, ss), 1.5, None, placement, "square")
    corners = {(1.5, 1.5), (5.5, 1.5), (5.5, 5.5), (1.5, 5.5)}
    assert (corners <= {tuple(p) for p in out.vertices.tolist()}) == (placement == "quadric")


# ---- the fixtures through both extractors ---------------------------------------------------------------------------------

FIELDS = {"sphere": (lambda: S.sphere_field()[0], [24, 24, 24]), "3d": (M.fixture_3d, M.FIXTURE_3D_SIZES),
          "2d": (M.fixture_2d, M.FIXTURE_2D_SIZES)}


@pytest.mark.parametrize("method", ["iso", "dual"])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_extracted_meshes(fi, name, method):
    make, sizes = FIELDS[name]
    mesh = (fi.iso_surface if method == "iso" else fi.dual_contour)(make(), sizes)
    assert len(mesh.indices) > 100
    for cell in (0.5, 1, 2, 3):
        for origin in ORIGINS:
            for placement in PLACEMENTS:
                out, _vm, _r = _check(fi, mesh, cell, origin, placement, "%s %s" % (name, method))
                assert len(out.indices) <= len(mesh.indices)


# ---- beyond one sort block and one workgroup ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def large(fi):
    f, _c = S.sphere_field(96, 44.0)
    mesh = fi.iso_surface(f, [96, 96, 96])
    assert len(mesh.indices) > 70000 and len(mesh.vertices) > 2 * 16384        # several sort blocks, hundreds of workgroups
    return mesh


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_large_sphere(fi, large, placement):
    out, _vm, ref = _check(fi, large, 2.0, ORIGINS[1], placement, "96^3")
    assert ref.fallbacks == 0 and R.euler_characteristic(len(out.vertices), out.indices) == 2


def test_repeated_calls_return_the_same_bytes(fi, large):
    first = fi.simplify_mesh(large, 3.0, vertex_map=True)
    for _ in range(3):
        again = fi.simplify_mesh(large, 3.0, vertex_map=True)
        _same_mesh(first[0], again[0])
        assert np.array_equal(first[1], again[1])


# ---- composition ------------------------------------------------------------------------------------------------------------

def test_parts_and_surface_index_of_a_result(fi, sphere):
    v, t = S.cube_mesh(12, 2.25, 0.75)
    cube = fi.simplify_mesh(_mesh(fi, v, t), 2.0)
    parts = fi.mesh_parts(cube)
    assert len(parts.size) == 1 and parts.closed[0] and parts.euler[0] == 2 and parts.primitives[0] == 192
    assert abs(parts.enclosed[0] - 729.0) < 1e-3 and abs(parts.size[0] - 486.0) < 1e-3
    mesh, centre = sphere
    coarse = fi.simplify_mesh(mesh, 3.0)
    index = fi.SurfaceIndex.from_mesh(coarse)
    d = index.distance(np.concatenate([coarse.vertices, centre[None, :].astype(np.float32)]))
    assert d[:-1].max() <= 1e-4 and abs(d[-1] - 9.0) < 0.5


@pytest.mark.parametrize("method", ["iso", "dual"])
def test_simplify_keyword_of_the_extractors(fi, method):
    f, sizes = M.fixture_3d(), M.FIXTURE_3D_SIZES
    ctx = fi.LatticeField(sizes)
    entries = [lambda **kw: (fi.iso_surface if method == "iso" else fi.dual_contour)(f, sizes, **kw),
               lambda **kw: (ctx.iso_surface if method == "iso" else ctx.dual_contour)(solution=f, **kw)]
    for call in entries:
        plain = call()
        _same_mesh(plain, call(simplify=None))                  # the default: what the call returned before it had the keyword
        _same_mesh(call(largest=1, parts=True)[0], call(largest=1, parts=True, simplify=None)[0])
        _same_mesh(call(simplify=2.0), fi.simplify_mesh(plain, 2.0))
        _same_mesh(call(simplify=(2.0, "mean")), fi.simplify_mesh(plain, 2.0, placement="mean"))
        _same_mesh(call(simplify=1.5, normals=False), fi.simplify_mesh(plain, 1.5)._replace(normals=None))
        coarse, parts = call(simplify=(2.0, "quadric"), largest=1, parts=True)
        _same_mesh(coarse, fi.simplify_mesh(call(largest=1), 2.0))
        want = fi.mesh_parts(coarse)                            # parts=True describes the mesh returned
        for a, b in zip(parts, want):
            assert np.array_equal(_bytes(a), _bytes(b))
        assert len(parts.size) == 1 and 0 < len(coarse.indices) < len(plain.indices) / 2
    with pytest.raises(ValueError):
        entries[0](simplify=(2.0, "median"))
    with pytest.raises(fi.FiError):
        entries[0](simplify=-1.0)


# ---- device pointers ------------------------------------------------------------------------------------------------------

def test_device_pointers(fi, sphere, tmp_path):
    """torch device tensors in and out (a fresh process, tests/simplify_torch_worker.py: torch stays out of this one): the host
    path's answers"""
    mesh, _c = sphere
    f, sizes = M.fixture_3d(), M.FIXTURE_3D_SIZES
    np.savez(tmp_path / "in.npz", sizes=np.array(sizes), f=f, **{k: v for k, v in zip(mesh._fields, mesh)})
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "simplify_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"].all()
    want, vmap = fi.simplify_mesh(mesh, 2.0, origin=ORIGINS[1], vertex_map=True)
    _same_mesh([o["quadric_" + k] for k in mesh._fields], want)
    assert np.array_equal(o["quadric_map"], vmap) and o["quadric_map"].dtype == np.int32
    bare = fi.simplify_mesh(mesh._replace(normals=None, keys=None), 3.0, placement="mean")
    assert o["mean_has_normals"][0] == 0
    _same_mesh([o["mean_" + k] for k in ("vertices", "indices", "keys")], [bare.vertices, bare.indices, bare.keys])
    _same_mesh([o["field_" + k] for k in mesh._fields], fi.iso_surface(f, sizes, largest=1, simplify=2.0))


# ---- every error code -------------------------------------------------------------------------------------------------

def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    INVALID = 1
    v = np.array([[0.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.5, 2.5, 0.5], [0.5, 0.5, 2.5]], np.float32)
    idx = np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    h, out = C.c_void_p(), C.c_void_p()

    def create(vertices):
        vertices = np.ascontiguousarray(vertices, np.float32)
        assert L.fi_mesh_create(C.byref(h), 3, 4, C.c_void_p(vertices.ctypes.data), None, None, 2, C.c_void_p(idx.ctypes.data), _capi.FI_HOST) == 0

    def simplify(cell=1.0, origin=None, placement=0, vmap=None, memory=_capi.FI_HOST, mesh=None):
        out.value = 12345
        return L.fi_mesh_simplify(h if mesh is None else mesh, cell, origin, placement, vmap, memory, C.byref(out))

    create(v)
    try:
        for cell in (0.0, -1.0, float("nan")):
            assert simplify(cell=cell) == INVALID and not out.value and L.fi_last_error()
        for placement in (-1, 2):
            assert simplify(placement=placement) == INVALID and not out.value
        assert simplify(memory=7) == INVALID and not out.value
        assert simplify(cell=1e-7) == INVALID and not out.value          # 0.5 / 1e-7 cells from the origin
        assert L.fi_mesh_simplify(h, 1.0, None, 0, None, _capi.FI_HOST, None) == INVALID
        far = (C.c_float * 3)(-3e6, 0.0, 0.0)
        assert simplify(origin=far) == INVALID and not out.value
        vmap = np.full(4, 7, np.int32)
        assert simplify(vmap=C.c_void_p(vmap.ctypes.data)) == 0 and out.value and vmap.tolist() == [0, 1, 2, 3]
        # no normals went in: none come out
        n = np.empty((4, 3), np.float32)
        assert L.fi_mesh_copy(out, None, C.c_void_p(n.ctypes.data), None, None, _capi.FI_HOST) == INVALID
        keys = np.empty(4, np.int64)
        assert L.fi_mesh_copy(out, None, None, None, C.c_void_p(keys.ctypes.data), _capi.FI_HOST) == 0 and np.all(np.diff(keys) > 0)
        L.fi_mesh_destroy(out)
    finally:
        L.fi_mesh_destroy(h)
    for bad in (np.nan, np.inf):
        w = v.copy()
        w[2, 1] = bad
        create(w)
        try:
            assert simplify() == INVALID and not out.value and L.fi_last_error()
        finally:
            L.fi_mesh_destroy(h)
    assert simplify(mesh=C.c_void_p()) == INVALID and not out.value
    with pytest.raises(ValueError):
        fi.simplify_mesh(fi.IsoMesh(v, None, idx, None), 1.0, placement="median")
    with pytest.raises(ValueError):
        fi.simplify_mesh(fi.IsoMesh(v, None, idx, None), 1.0, origin=[0.0, 0.0])
