"""The connected parts of a mesh on the device (fi_parts.hip through fi_mesh_create / fi_mesh_parts / fi_mesh_measure /
fi_mesh_select) against the numpy restatement of the contract (tests/mesh_parts_reference.py): labels, every integer column,
the bounding boxes and every array of a selection bit-equal; size and enclosed within (P_c + 16) 2^-52 M_c of the terms summed
by math.fsum -- the bound of any summation order plus the terms' own roundings."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import iso_reference as R
import mesh_parts_reference as M

pytestmark = pytest.mark.gpu

INTS = ("vertices", "primitives", "edges", "boundary", "irregular")


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _agree(got, mesh, what=""):
    """got: MeshParts of `mesh` from the device -> the reference's Parts"""
    ref = M.Parts(mesh.vertices, mesh.indices)
    assert len(got.size) == ref.count, what
    assert got.vertex_labels.dtype == np.int32 and got.primitive_labels.dtype == np.int32
    assert np.array_equal(got.vertex_labels, ref.vertex_labels), what
    assert np.array_equal(got.primitive_labels, ref.primitive_labels), what
    for name in INTS:
        assert np.array_equal(getattr(got, name), getattr(ref, name)), (what, name)
    assert np.array_equal(got.closed, ref.closed) and np.array_equal(got.euler, ref.euler), what
    if ref.count:
        assert np.array_equal(_bits(got.lo), _bits(ref.lo)) and np.array_equal(_bits(got.hi), _bits(ref.hi)), what
        ds, de = np.abs(got.size - ref.size), np.abs(got.enclosed - ref.enclosed)
        print("%s parts %d  size error / bound %.3g  enclosed error / bound %.3g" % (
            what, ref.count, (ds / np.maximum(ref.size_bound, 1e-300)).max(), (de / np.maximum(ref.enclosed_bound, 1e-300)).max()))
        assert (ds <= ref.size_bound).all(), (what, ds, ref.size_bound)
        assert (de <= ref.enclosed_bound).all(), (what, de, ref.enclosed_bound)
    return ref


def _same_mesh(a, b):
    for u, w in zip(a, b):
        assert (u is None) == (w is None)
        if u is not None:
            assert u.dtype == w.dtype and u.shape == w.shape and np.array_equal(u.view(np.uint8), w.view(np.uint8))


def _selected(mesh, ref, keep):
    return M.select(mesh.vertices, mesh.normals, mesh.indices, mesh.keys, ref.vertex_labels, ref.primitive_labels, keep)


# ---- every cell case ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ndim", [2, 3])
def test_every_cell_case(fi, ndim):
    mags = np.array([0.3, 0.7, 1.1, 0.5, 0.9, 0.4, 1.3, 0.6], np.float32)[:1 << ndim]
    for case in range(1 << (1 << ndim)):
        f = np.array([-1.0 if (case >> k) & 1 else 1.0 for k in range(1 << ndim)], np.float32) * mags
        mesh, parts = fi.iso_surface(f, [2] * ndim, parts=True)
        assert len(mesh.indices) == len(R.cell_primitives(ndim, R.case_inside(ndim, case)))
        _agree(parts, mesh, "case %d" % case)


# ---- the fixtures, both extractors, both signs ----------------------------------------------------------------------------

FIELDS = {"3d": (M.fixture_3d, M.FIXTURE_3D_SIZES), "2d": (M.fixture_2d, M.FIXTURE_2D_SIZES),
          "checkerboard": (M.checkerboard, M.CHECKERBOARD_SIZES)}


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("method", ["iso", "dual"])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_fixtures(fi, name, method, sign):
    make, sizes = FIELDS[name]
    f = (sign * make()).astype(np.float32)
    mesh, parts = (fi.iso_surface if method == "iso" else fi.dual_contour)(f, sizes, parts=True)
    ref = _agree(parts, mesh, "%s %s %+d" % (name, method, sign))
    _same_mesh(mesh, (fi.iso_surface if method == "iso" else fi.dual_contour)(f, sizes))
    if method != "iso":
        return
    # what tests/test_mesh_parts_reference.py found for these meshes on the host
    if name == "3d":
        assert list(zip(ref.vertices, ref.primitives, ref.edges)) == [(148, 252, 399), (310, 616, 924), (512, 1024, 1536), (100, 196, 294)]
        assert list(parts.boundary) == [42, 0, 0, 0] and list(parts.euler) == [1, 2, 0, 2] and not parts.irregular.any()
        assert np.allclose(sign * parts.enclosed[1:], [278.44, 308.89, 45.245], rtol=0, atol=[0.005, 0.005, 0.0005])
    elif name == "2d":
        assert len(mesh.vertices) == 113 and len(mesh.indices) == 112 and list(parts.boundary) == [2, 0, 0, 0]
        assert np.allclose(sign * parts.enclosed[1:], [116.24, -17.44, 31.52], rtol=0, atol=0.005)
    elif sign == 1:
        assert (len(mesh.vertices), len(mesh.indices), len(parts.size)) == (1321, 1344, 252) and (parts.vertex_labels >= 0).all()


def test_empty_mesh_and_constant_field(fi):
    for sizes in ([6, 5], [6, 5, 4]):
        mesh, parts = fi.iso_surface(np.full(int(np.prod(sizes)), 2.0, np.float32), sizes, parts=True, largest=3)
        assert len(mesh.vertices) == 0 and len(mesh.indices) == 0 and len(parts.size) == 0 and len(parts.vertex_labels) == 0
        nd = len(sizes)
        empty = fi.IsoMesh(np.empty((0, nd), np.float32), None, np.empty((0, nd), np.int32), None)
        p = fi.mesh_parts(empty)
        assert len(p.size) == 0 and p.lo.shape == (0, nd) and len(p.primitive_labels) == 0
        out = fi.select_parts(empty, [])
        assert len(out.vertices) == 0 and len(out.indices) == 0 and out.normals is None
        # vertices without primitives: no part, every label -1
        lone = fi.IsoMesh(np.ones((3, nd), np.float32), None, np.empty((0, nd), np.int32), None)
        p = fi.mesh_parts(lone)
        assert len(p.size) == 0 and list(p.vertex_labels) == [-1, -1, -1]


# ---- meshes the caller brings -----------------------------------------------------------------------------------------

def _caller(fi, v, idx, normals=None, keys=None):
    return fi.IsoMesh(np.asarray(v, np.float32), normals, np.asarray(idx, np.int32), keys)


def test_triangle_soup(fi):
    rng = np.random.default_rng(1)
    n = 700                                                    # (more than one workgroup of primitives)
    mesh = _caller(fi, rng.normal(size=(3 * n, 3)) * 5, rng.permutation(3 * n).reshape(n, 3))
    parts = fi.mesh_parts(mesh)
    _agree(parts, mesh, "soup")
    assert len(parts.size) == n and (parts.primitives == 1).all() and (parts.boundary == 3).all() and (parts.euler == 1).all()
    # coincident positions under different indices do not join
    twin = _caller(fi, np.tile(rng.normal(size=(3, 3)), (2, 1)), [[0, 1, 2], [3, 4, 5]])
    assert list(fi.mesh_parts(twin).primitive_labels) == [0, 1]


def test_unused_vertices_and_repeated_indices(fi):
    rng = np.random.default_rng(2)
    v = rng.normal(size=(12, 3))
    nrm = rng.normal(size=(12, 3)).astype(np.float32)
    keys = (np.arange(12, dtype=np.int64) * 7 + 3)
    mesh = _caller(fi, v, [[9, 4, 4], [1, 2, 10], [10, 2, 1], [7, 7, 7], [4, 11, 9]], nrm, keys)
    parts = fi.mesh_parts(mesh)
    ref = _agree(parts, mesh, "unused")
    assert list(parts.vertex_labels) == [-1, 0, 0, -1, 1, -1, -1, 2, -1, 1, 0, 1]
    assert list(parts.vertices) == [3, 3, 1] and list(parts.edges) == [3, 3, 0] and list(parts.closed) == [True, False, True]
    for keep in ([True, True, True], [False, True, False], [True, False, True]):
        _same_mesh(fi.select_parts(mesh, keep), _selected(mesh, ref, keep))
    assert len(fi.select_parts(mesh, [True] * 3).vertices) == 7          # the unused vertices are dropped
    # without normals and keys: the keys are 0 .. V-1, a selection has no normals either
    bare = _caller(fi, v, mesh.indices)
    out = fi.select_parts(bare, [False, True, False])
    assert out.normals is None and list(out.keys) == [4, 9, 11] and out.indices.tolist() == [[1, 0, 0], [0, 2, 1]]
    # 2-D: a fork, a loop through a repeated index, an isolated segment of equal ends
    flat = _caller(fi, rng.normal(size=(9, 2)), [[0, 1], [1, 2], [1, 3], [4, 4], [5, 6], [6, 5], [8, 8]])
    p2 = fi.mesh_parts(flat)
    _agree(p2, flat, "fork")
    assert list(p2.boundary) == [3, 0, 0, 0] and list(p2.irregular) == [1, 1, 0, 1] and list(p2.vertex_labels) == [0, 0, 0, 0, 1, 2, 2, -1, 3]


def test_shared_vertex_and_same_direction(fi):
    tet = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float32)
    second = np.array([0, 4, 5, 6])[tet]
    mesh = _caller(fi, v, np.concatenate([tet, second]))
    parts = fi.mesh_parts(mesh)
    _agree(parts, mesh, "two tetrahedra")
    assert len(parts.size) == 1 and parts.closed[0] and parts.euler[0] == 3 and parts.vertices[0] == 7 and parts.edges[0] == 12
    fan = _caller(fi, np.random.default_rng(3).normal(size=(4, 3)), [[0, 1, 2], [0, 1, 3]])
    pf = fi.mesh_parts(fan)
    _agree(pf, fan, "same direction")
    assert list(pf.irregular) == [1] and list(pf.boundary) == [4] and list(pf.edges) == [5] and not pf.closed[0]


def test_merged_slab_pieces(fi):
    f, sizes = M.fixture_3d(), M.FIXTURE_3D_SIZES
    pieces = fi.LatticeGroup(sizes, 2).iso_surface(f)
    for k, piece in enumerate(pieces):                         # a piece is just a mesh: its parts are its own
        _agree(fi.mesh_parts(piece), piece, "piece %d" % k)
    merged = fi.merge_meshes(pieces)
    one, whole = fi.iso_surface(f, sizes, parts=True)
    got = fi.mesh_parts(merged)
    _agree(got, merged, "merged")
    # the merged mesh is the undivided one, so the exact columns agree (the sums too, but only the restatement binds them)
    assert np.array_equal(merged.keys, one.keys) and np.array_equal(got.vertex_labels, whole.vertex_labels)
    for name in INTS:
        assert np.array_equal(getattr(got, name), getattr(whole, name)), name
    assert np.array_equal(_bits(got.lo), _bits(whole.lo)) and np.array_equal(_bits(got.hi), _bits(whole.hi))


# ---- beyond one workgroup, deep parent chains -----------------------------------------------------------------------

def test_long_permuted_chain(fi):
    n = 200000
    rng = np.random.default_rng(7)
    perm = rng.permutation(n + 1)
    idx = np.stack([perm[:-1], perm[1:]], axis=1).astype(np.int32)
    v = rng.normal(size=(n + 1, 2)).astype(np.float32)
    for name, chain in (("chain", idx), ("reversed", np.ascontiguousarray(idx[::-1, ::-1]))):
        mesh = _caller(fi, v, chain)
        parts = fi.mesh_parts(mesh)
        _agree(parts, mesh, name)
        assert len(parts.size) == 1 and parts.boundary[0] == 2 and parts.irregular[0] == 0 and parts.edges[0] == n


@pytest.fixture(scope="module")
def spheres(fi):
    """5 x 5 x 5 spheres on 96^3: the mesh, its parts from the device, the reference's"""
    n, r = 96, 6.2
    c = 9.6 + 19.2 * np.arange(5)
    ax = np.arange(n, dtype=np.float64)
    d1 = np.abs(ax[:, None] - c[None, :]).min(axis=1)
    f = (np.sqrt(d1[:, None, None] ** 2 + d1[None, :, None] ** 2 + d1[None, None, :] ** 2) - r).astype(np.float32).reshape(-1)
    mesh, parts = fi.iso_surface(f, [n, n, n], parts=True)
    return mesh, parts, _agree(parts, mesh, "spheres")


def test_many_spheres(fi, spheres):
    mesh, parts, ref = spheres
    assert len(parts.size) == 125 and parts.closed.all() and (parts.euler == 2).all() and (parts.vertex_labels >= 0).all()
    assert parts.primitives.min() > 2 * 256                    # every part spans several chunks of the measuring pass
    assert np.allclose(parts.enclosed, 4.0 / 3.0 * np.pi * 6.2 ** 3, rtol=0.05)


def test_measures_repeat_bit_for_bit(fi, spheres):
    mesh, parts, _ref = spheres
    for _ in range(5):                                         # (a new handle each time: everything is computed again)
        again = fi.mesh_parts(mesh)
        for a, b in zip(parts, again):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- select ---------------------------------------------------------------------------------------------------------------

def test_select_on_the_checkerboard(fi):
    mesh, parts = fi.iso_surface(M.checkerboard(), M.CHECKERBOARD_SIZES, parts=True)
    ref = _agree(parts, mesh, "checkerboard")
    n = len(parts.size)
    _same_mesh(fi.select_parts(mesh, np.ones(n, bool)), mesh)         # no unused vertex: the same arrays
    none = fi.select_parts(mesh, np.zeros(n, bool))
    assert len(none.vertices) == 0 and len(none.indices) == 0 and none.indices.shape[1] == 3
    masks = [np.arange(n) == c for c in range(n)] + [np.random.default_rng(4).random(n) < 0.4]
    for keep in masks:
        _same_mesh(fi.select_parts(mesh, keep), _selected(mesh, ref, keep))
    with pytest.raises(fi.FiError) as e:
        fi.select_parts(mesh, np.ones(n + 1, bool))
    assert e.value.code == 1


def test_keep_parts_rules(fi):
    mesh, parts = fi.iso_surface(M.fixture_3d(), M.FIXTURE_3D_SIZES, parts=True)
    assert list(fi.keep_parts(parts, largest=1)) == [False, False, True, False]       # the torus: the largest area
    assert abs(parts.size[2] - 339.2) < 0.05
    assert list(fi.keep_parts(parts, closed=True)) == [False, True, True, True]
    assert list(fi.keep_parts(parts, closed=False, largest=2)) == [True, False, False, False]
    assert list(fi.keep_parts(parts, min_primitives=253)) == [False, True, True, False]
    assert list(fi.keep_parts(parts, min_size=float(parts.size[1]))) == [False, True, True, False]
    assert list(fi.keep_parts(parts, largest=0)) == [False] * 4 and fi.keep_parts(parts).all()
    tie = parts._replace(size=np.array([1.0, 3.0, 3.0, 2.0]))
    assert list(fi.keep_parts(tie, largest=1)) == [False, True, False, False]         # ties go to the lower number


@pytest.mark.parametrize("method", ["iso", "dual"])
def test_extract_and_filter_in_one_call(fi, method):
    f, sizes = M.fixture_3d(), M.FIXTURE_3D_SIZES
    ctx = fi.LatticeField(sizes)
    call = ctx.iso_surface if method == "iso" else ctx.dual_contour
    plain = call(solution=f)
    _same_mesh(plain, (fi.iso_surface if method == "iso" else fi.dual_contour)(f, sizes))
    if method == "iso":
        v, n, idx, keys = R.extract(f, sizes)                  # what the call returned before it had the keywords
        assert np.array_equal(plain.keys, keys) and np.array_equal(plain.indices, idx)
        assert np.array_equal(_bits(plain.vertices), _bits(v)) and np.abs(plain.normals - n).max() <= 1e-5
    mesh, parts = call(solution=f, largest=1, parts=True)
    whole = fi.mesh_parts(plain)
    _same_mesh(mesh, fi.select_parts(plain, fi.keep_parts(whole, largest=1)))
    _agree(parts, mesh, "largest of " + method)
    assert len(parts.size) == 1
    small = call(solution=f, min_size=float(np.sort(whole.size)[-2]), normals=False)
    assert small.normals is None
    keep = whole.size >= np.sort(whole.size)[-2]
    _same_mesh(small, fi.select_parts(plain, keep)._replace(normals=None))
    assert keep.sum() == 2


# ---- device pointers ------------------------------------------------------------------------------------------------------

def test_device_pointers(fi, tmp_path):
    """torch device tensors in, labels out as device tensors (a fresh process, tests/parts_torch_worker.py: torch stays out of
    this one): the host path's answers"""
    f, sizes = M.fixture_3d(), M.FIXTURE_3D_SIZES
    mesh, parts = fi.iso_surface(f, sizes, parts=True)
    keep = np.array([True, False, True, False])
    np.savez(tmp_path / "in.npz", sizes=np.array(sizes), f=f, keep=keep, **{k: v for k, v in zip(mesh._fields, mesh)})
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "parts_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["labels_on_device"][0] and o["selection_on_device"][0]
    for prefix in ("parts_", "field_parts_"):
        for name, want in zip(parts._fields, parts):
            got = o[prefix + name]
            assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), prefix + name
    _same_mesh([o["selected_" + k] for k in mesh._fields], fi.select_parts(mesh, keep))
    _same_mesh([o["largest_" + k] for k in mesh._fields], fi.iso_surface(f, sizes, largest=1))


# ---- every error code -------------------------------------------------------------------------------------------------

def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    INVALID, UNSUPPORTED = 1, 5
    v = np.zeros((4, 3), np.float32)
    idx = np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    pv, pi = C.c_void_p(v.ctypes.data), C.c_void_p(idx.ctypes.data)
    h = C.c_void_p()
    for ndim in (1, 4, 0):
        assert L.fi_mesh_create(C.byref(h), ndim, 4, pv, None, None, 2, pi, _capi.FI_HOST) == UNSUPPORTED and not h.value
    assert L.fi_mesh_create(C.byref(h), 3, 2 ** 31, pv, None, None, 2, pi, _capi.FI_HOST) == UNSUPPORTED and not h.value
    assert L.fi_mesh_create(C.byref(h), 3, 4, pv, None, None, 2 ** 31, pi, _capi.FI_HOST) == UNSUPPORTED and not h.value
    assert L.fi_mesh_create(C.byref(h), 3, -1, pv, None, None, 2, pi, _capi.FI_HOST) == INVALID and not h.value
    assert L.fi_mesh_create(C.byref(h), 3, 4, pv, None, None, 2, pi, 7) == INVALID and not h.value
    for bad in (4, -1):
        wrong = idx.copy()
        wrong[1, 2] = bad
        assert L.fi_mesh_create(C.byref(h), 3, 4, pv, None, None, 2, C.c_void_p(wrong.ctypes.data), _capi.FI_HOST) == INVALID
        assert not h.value and L.fi_last_error()
    assert L.fi_mesh_create(C.byref(h), 3, 4, pv, None, None, 2, pi, _capi.FI_HOST) == 0 and h.value
    try:
        # no normals were given: fi_mesh_copy refuses a normals buffer, and copies the rest
        n = np.empty((4, 3), np.float32)
        keys = np.empty(4, np.int64)
        assert L.fi_mesh_copy(h, None, C.c_void_p(n.ctypes.data), None, None, _capi.FI_HOST) == INVALID
        assert L.fi_mesh_copy(h, None, None, None, C.c_void_p(keys.ctypes.data), _capi.FI_HOST) == 0 and list(keys) == [0, 1, 2, 3]
        count = C.c_long(-1)
        assert L.fi_mesh_parts(h, C.byref(count), None, None, _capi.FI_HOST) == 0 and count.value == 1
        assert L.fi_mesh_parts(h, C.byref(count), None, None, 7) == INVALID
        rows = (_capi.FiMeshPart * 2)()
        rows[0].vertices = -5
        count = C.c_long(-1)
        assert L.fi_mesh_measure(h, 0, C.cast(rows, C.c_void_p), C.byref(count)) == INVALID      # too little room: the count,
        assert count.value == 1 and rows[0].vertices == -5                                       # nothing written
        assert L.fi_mesh_measure(h, 0, None, C.byref(count)) == INVALID and count.value == 1
        assert L.fi_mesh_measure(h, 2, C.cast(rows, C.c_void_p), C.byref(count)) == 0 and rows[0].vertices == 4
        first = bytes(rows)[:C.sizeof(_capi.FiMeshPart)]
        assert L.fi_mesh_measure(h, 1, C.cast(rows, C.c_void_p), None) == 0 and bytes(rows)[:len(first)] == first
        out = C.c_void_p()
        keep = (C.c_ubyte * 2)(1, 1)
        assert L.fi_mesh_select(h, 2, keep, C.byref(out)) == INVALID and not out.value
        assert L.fi_mesh_select(h, 0, keep, C.byref(out)) == INVALID and not out.value
        assert L.fi_mesh_select(h, 1, keep, C.byref(out)) == 0 and out.value
        assert L.fi_mesh_copy(out, None, C.c_void_p(n.ctypes.data), None, None, _capi.FI_HOST) == INVALID
        L.fi_mesh_destroy(out)
    finally:
        L.fi_mesh_destroy(h)
    assert L.fi_mesh_parts(None, C.byref(count), None, None, _capi.FI_HOST) == INVALID
    assert L.fi_mesh_measure(None, 0, None, C.byref(count)) == INVALID
    assert L.fi_mesh_select(None, 0, None, C.byref(out)) == INVALID
    assert L.fi_mesh_create(None, 3, 4, pv, None, None, 2, pi, _capi.FI_HOST) == INVALID
