"""Mesh smoothing on the device (fi_smooth.hip through fi_mesh_smooth / fi_mesh_normals, smooth_mesh, mesh_normals and the
extractors' smooth keyword) against the numpy restatement of the contract (tests/smooth_reference.py): every output array --
positions, normals, indices, keys -- bit for bit."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import iso_reference as R
import mesh_parts_reference as M
import simplify_reference as S
import smooth_cases as K
import smooth_reference as T

pytestmark = pytest.mark.gpu

BOUNDARIES = ("fixed", "slide", "free")
NORMALS = ("recompute", "keep")


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


def _mesh(fi, v, idx, normals=None, keys=None):
    v = np.asarray(v, np.float32)
    return fi.IsoMesh(v, normals, np.asarray(idx, np.int32).reshape(-1, v.shape[1]), keys)


def _check(fi, mesh, iterations=10, lam=0.5, mu=-0.53, boundary="fixed", max_move=None, normals="recompute", what=""):
    """smooth_mesh of an IsoMesh of numpy arrays against the restatement -> the device's mesh"""
    what = "%s: %d iterations, lam %g mu %g, %s, max_move %s, %s" % (what, iterations, lam, mu, boundary, max_move, normals)
    want_v, want_n = T.smooth(mesh.vertices, mesh.normals, mesh.indices, iterations, lam, mu, T.BOUNDARY[boundary],
                              0.0 if max_move is None else max_move, T.NORMALS[normals])
    out = fi.smooth_mesh(mesh, iterations, lam, mu, boundary, max_move, normals)
    assert out.vertices.dtype == np.float32 and out.vertices.shape == want_v.shape, what
    diff = np.flatnonzero((out.vertices.view(np.uint32) != want_v.view(np.uint32)).any(axis=1))
    assert len(diff) == 0, (what, len(diff), diff[:3], out.vertices[diff[:3]], want_v[diff[:3]])
    assert (out.normals is None) == (want_n is None), what
    if want_n is not None:
        diff = np.flatnonzero((out.normals.view(np.uint32) != want_n.view(np.uint32)).any(axis=1))
        assert len(diff) == 0, (what, "normals", len(diff), diff[:3], out.normals[diff[:3]], want_n[diff[:3]])
    assert out.indices.dtype == np.int32 and np.array_equal(out.indices, mesh.indices), what
    keys = np.arange(len(mesh.vertices), dtype=np.int64) if mesh.keys is None else mesh.keys
    assert out.keys.dtype == np.int64 and np.array_equal(out.keys, keys), what
    return out


def _check_normals(fi, mesh, what=""):
    out = fi.mesh_normals(mesh)
    want = T.mesh_normals(mesh.vertices, mesh.indices)
    assert out.normals is not None and np.array_equal(_bytes(out.normals), _bytes(want)), what
    keys = np.arange(len(mesh.vertices), dtype=np.int64) if mesh.keys is None else mesh.keys
    _same_mesh(out._replace(normals=None), mesh._replace(normals=None, keys=keys))
    return out


# ---- the cases of tests/test_smooth_reference.py ------------------------------------------------------------------------

@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_constructed_cases(fi, boundary):
    grid = K.flat_grid(6, 3.125)
    cases = K.constructed() + [("polygon",) + K.polygon(), ("flat grid", grid[0], grid[1])]
    for name, v, t in cases:
        mesh = _mesh(fi, v, t)
        for mu, max_move in ((0.0, None), (-0.53, None), (-0.53, 0.05)):
            _check(fi, mesh, 3, 0.5, mu, boundary, max_move, what=name)
        _check(fi, mesh, 0, boundary=boundary, what=name)
        made = _check_normals(fi, mesh, name)
        _check(fi, made, 2, boundary=boundary, normals="recompute", what=name + " with normals")
        _check(fi, made, 2, boundary=boundary, normals="keep", what=name + " with normals")
    # an unused vertex may be anything, and keeps it
    name, v, t = K.constructed()[5]
    v = v.copy()
    v[6] = [np.nan, np.inf, -np.inf]
    out = _check(fi, _mesh(fi, v, t), 4, boundary=boundary, what="unused NaN")
    assert np.array_equal(_bytes(out.vertices[4:]), _bytes(v[4:]))
    _check_normals(fi, _mesh(fi, v, t), "unused NaN")


def test_polygon_and_flat_grid_answers(fi):
    v, seg = K.polygon()
    out = _check(fi, _mesh(fi, v, seg), 7, 0.5, -0.53, "free", what="polygon")
    s = 1.0 - np.cos(2.0 * np.pi / 12)
    want = 5.0 * ((1.0 - 0.5 * s) * (1.0 - float(np.float32(-0.53)) * s)) ** 7
    r = np.sqrt(((out.vertices.astype(np.float64) - out.vertices.astype(np.float64).mean(axis=0)) ** 2).sum(axis=1))
    assert np.abs(r - want).max() <= 4e-6
    v, t, _rim = K.flat_grid(6, 3.125)
    out = _check(fi, _mesh(fi, v, t), 5, what="flat grid")
    assert np.array_equal(_bytes(out.vertices), _bytes(v))


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_cut_sphere(fi, boundary):
    pos, nrm, idx, keys = K.cut_sphere()
    mesh = fi.IsoMesh(pos, nrm, idx, keys)
    out = _check(fi, mesh, 5, boundary=boundary, what="cut sphere")
    rim = T.adjacency(len(pos), idx, 3)[3]
    assert rim.sum() == 40
    if boundary == "slide":
        assert np.array_equal(_bytes(out.vertices[rim, 0]), _bytes(pos[rim, 0])) and not np.array_equal(out.vertices[rim], pos[rim])
    if boundary == "fixed":
        assert np.array_equal(_bytes(out.vertices[rim]), _bytes(pos[rim]))


@pytest.fixture(scope="module")
def stairs(fi):
    (pos, nrm, idx, keys), centre = K.staircase()
    return fi.IsoMesh(pos, nrm, idx, keys), centre


@pytest.mark.parametrize("mu", [0.0, -0.53])
def test_staircase(fi, stairs, mu):
    mesh, centre = stairs
    out = _check(fi, mesh, 10, 0.5, mu, what="staircase")
    assert K.radial_rms_angle(out.vertices, out.indices, centre) < 0.5 * K.radial_rms_angle(mesh.vertices, mesh.indices, centre)
    for max_move in (0.5, 0.25):
        out = _check(fi, mesh, 10, 0.5, mu, "fixed", max_move, what="staircase")
        moved = np.sqrt(((out.vertices.astype(np.float64) - mesh.vertices.astype(np.float64)) ** 2).sum(axis=1))
        assert moved.max() <= max_move + 2.0 * float(np.spacing(np.abs(out.vertices).max()))


# ---- the fixtures through both extractors ---------------------------------------------------------------------------------

FIELDS = {"sphere": (lambda: S.sphere_field()[0], [24, 24, 24]), "3d": (M.fixture_3d, M.FIXTURE_3D_SIZES),
          "2d": (M.fixture_2d, M.FIXTURE_2D_SIZES)}


@pytest.mark.parametrize("method", ["iso", "dual"])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_extracted_meshes(fi, name, method):
    make, sizes = FIELDS[name]
    mesh = (fi.iso_surface if method == "iso" else fi.dual_contour)(make(), sizes)
    assert len(mesh.indices) > 100
    for iterations, boundary, mu, max_move, normals in itertools.product((1, 5), BOUNDARIES, (0.0, -0.53), (None, 0.5), NORMALS):
        _check(fi, mesh, iterations, 0.5, mu, boundary, max_move, normals, "%s %s" % (name, method))
    _check_normals(fi, mesh._replace(normals=None), "%s %s" % (name, method))


def test_normals_agree_with_the_extractors(fi):
    f, _c = S.sphere_field()
    mesh = fi.iso_surface(f, [24, 24, 24])
    assert (fi.mesh_normals(mesh).normals.astype(np.float64) * mesh.normals).sum(axis=1).min() >= 0.995
    mesh = fi.iso_surface(M.fixture_2d(), M.FIXTURE_2D_SIZES)
    assert (fi.mesh_normals(mesh).normals.astype(np.float64) * mesh.normals).sum(axis=1).min() >= 0.977


# ---- beyond one sort block and one workgroup ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def large(fi):
    f, _c = S.sphere_field(96, 44.0)
    mesh = fi.iso_surface(f, [96, 96, 96])
    assert (len(mesh.vertices), len(mesh.indices)) == (36520, 73036)           # 438 216 directed pairs: several sort blocks
    return mesh


@pytest.mark.parametrize("boundary,mu,max_move,normals", [("fixed", -0.53, None, "recompute"), ("free", 0.0, 0.3, "keep"),
                                                          ("slide", -0.53, 0.3, "recompute")])
def test_large_sphere(fi, large, boundary, mu, max_move, normals):
    _check(fi, large, 5, 0.5, mu, boundary, max_move, normals, "96^3")


def test_repeated_calls_return_the_same_bytes(fi, large):
    first = fi.smooth_mesh(large, 3, max_move=0.3)
    for _ in range(3):
        _same_mesh(first, fi.smooth_mesh(large, 3, max_move=0.3))
    made = fi.mesh_normals(large)
    _same_mesh(made, fi.mesh_normals(large))


# ---- where one piece of the arena runs into the next ----------------------------------------------------------------------

EDGE = (63, 64, 65)


@functools.lru_cache(maxsize=None)
def mesh_case(ndim, nv, npr):
    """nv vertices, npr primitives, after tests/test_gpu_mesh_scratch.py's: a strip (2-D: a polyline) over the first vertices
    with a few chords across it, two loose primitives on vertices of their own, the last vertex unused; the primitives
    shuffled.  -> (vertices, normals, indices)"""
    rng = np.random.default_rng(2000 * ndim + 10 * nv + npr)
    used = nv - 1
    body = used - 2 * ndim
    prims = [list(range(i, i + ndim)) if i % 2 == 0 or ndim == 2 else [i + 1, i, i + 2] for i in range(body - ndim + 1)]
    prims += [list(range(body + ndim * k, body + ndim * (k + 1))) for k in range(2)]
    extra = npr - len(prims)
    assert 0 < extra < 10
    prims += [[0, 2 * k + 2, 2 * k + 4][:ndim] for k in range(extra)]
    idx = np.array(prims, np.int32)[rng.permutation(npr)]
    assert idx.shape == (npr, ndim) and idx.max() == used - 1
    v = (rng.normal(size=(nv, ndim)) * 2.0).astype(np.float32)
    nrm = rng.normal(size=(nv, ndim))
    return v, (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32), idx


@pytest.mark.parametrize("ndim,nv,npr", [(ndim, nv, npr) for ndim in (3, 2) for nv in EDGE for npr in EDGE])
def test_arena_edges(fi, ndim, nv, npr):
    v, nrm, idx = mesh_case(ndim, nv, npr)
    mesh = fi.IsoMesh(v, nrm, idx, None)
    what = "%d-D, %d vertices, %d primitives" % (ndim, nv, npr)
    for boundary in BOUNDARIES:
        _check(fi, mesh, 3, 0.5, -0.53, boundary, 0.4, "recompute", what)
    _check(fi, mesh, 2, 0.5, 0.0, "free", None, "keep", what)
    _check_normals(fi, mesh._replace(normals=None), what)


# ---- composition ------------------------------------------------------------------------------------------------------------

def test_parts_simplify_and_surface_index_of_a_result(fi, stairs):
    mesh, centre = stairs
    faired = fi.smooth_mesh(mesh, 10)
    parts = fi.mesh_parts(faired)
    assert len(parts.size) == 1 and parts.closed[0] and parts.euler[0] == 2 and parts.primitives[0] == len(mesh.indices)
    assert abs(parts.enclosed[0] - R.signed_measure(faired.vertices, faired.indices)) < 1e-6 * parts.enclosed[0]
    coarse = fi.simplify_mesh(faired, 3.0)
    assert 0 < len(coarse.indices) < len(faired.indices) / 4 and len(fi.mesh_parts(coarse).size) == 1
    index = fi.SurfaceIndex.from_mesh(faired)
    d = index.distance(np.concatenate([faired.vertices, centre[None, :].astype(np.float32)]))
    assert d[:-1].max() <= 1e-4 and abs(d[-1] - 9.0) < 0.5


@pytest.mark.parametrize("method", ["iso", "dual"])
def test_smooth_keyword_of_the_extractors(fi, method):
    f, sizes = M.fixture_3d(), M.FIXTURE_3D_SIZES
    ctx = fi.LatticeField(sizes)
    entries = [lambda **kw: (fi.iso_surface if method == "iso" else fi.dual_contour)(f, sizes, **kw),
               lambda **kw: (ctx.iso_surface if method == "iso" else ctx.dual_contour)(solution=f, **kw)]
    options = {"iterations": 3, "lam": 0.6, "mu": 0.0, "boundary": "slide", "max_move": 0.3, "normals": "keep"}
    for call in entries:
        plain = call()
        _same_mesh(plain, call(smooth=None))                    # the default: what the call returned before it had the keyword
        _same_mesh(call(largest=1, parts=True)[0], call(largest=1, parts=True, smooth=None)[0])
        _same_mesh(call(simplify=2.0), call(simplify=2.0, smooth=None))
        _same_mesh(call(smooth=4), fi.smooth_mesh(plain, 4))
        _same_mesh(call(smooth=options), fi.smooth_mesh(plain, **options))
        _same_mesh(call(smooth=2, normals=False), fi.smooth_mesh(plain, 2)._replace(normals=None))
        _same_mesh(call(smooth=4, largest=1), fi.smooth_mesh(call(largest=1), 4))
        # parts selection -> smooth -> simplify; parts=True describes what is returned
        coarse, parts = call(smooth=4, simplify=2.0, largest=1, parts=True)
        _same_mesh(coarse, fi.simplify_mesh(fi.smooth_mesh(call(largest=1), 4), 2.0))
        want = fi.mesh_parts(coarse)
        for a, b in zip(parts, want):
            assert np.array_equal(_bytes(a), _bytes(b))
        assert len(parts.size) == 1 and 0 < len(coarse.indices) < len(plain.indices) / 2
    with pytest.raises(ValueError):
        entries[0](smooth={"boundary": "loose"})
    with pytest.raises(TypeError):
        entries[0](smooth={"steps": 3})
    with pytest.raises(fi.FiError):
        entries[0](smooth=-1)


def test_mesh_normals_of_a_mesh_without_normals(fi):
    pos, nrm, idx, keys = R.extract(M.fixture_3d(), M.FIXTURE_3D_SIZES)
    bare = fi.IsoMesh(pos, None, idx, None)
    assert fi.smooth_mesh(bare, 2).normals is None              # none went in: none come out ...
    made = _check_normals(fi, bare, "fixture")                  # ... but mesh_normals makes them
    assert np.array_equal(made.keys, np.arange(len(pos)))
    assert (made.normals.astype(np.float64) * nrm).sum(axis=1).min() > 0.5                # (they point the extractor's way)
    empty = fi.mesh_normals(fi.IsoMesh(np.zeros((0, 3), np.float32), None, np.zeros((0, 3), np.int32), None))
    assert empty.vertices.shape == (0, 3) and empty.normals.shape == (0, 3) and empty.indices.shape == (0, 3)
    loose = fi.mesh_normals(fi.IsoMesh(pos[:5], None, np.zeros((0, 3), np.int32), None))
    assert np.array_equal(_bytes(loose.vertices), _bytes(pos[:5])) and not loose.normals.any()
    same = fi.smooth_mesh(fi.IsoMesh(pos[:5], nrm[:5], np.zeros((0, 3), np.int32), None), 3)
    assert np.array_equal(_bytes(same.vertices), _bytes(pos[:5])) and not same.normals.any()
    empty = fi.smooth_mesh(fi.IsoMesh(np.zeros((0, 2), np.float32), None, np.zeros((0, 2), np.int32), None), 3)
    assert empty.vertices.shape == (0, 2) and empty.normals is None


# ---- device pointers ------------------------------------------------------------------------------------------------------

def test_device_pointers(fi, tmp_path):
    """torch device tensors in and out (a fresh process, tests/smooth_torch_worker.py: torch stays out of this one): the host
    path's answers"""
    mesh = fi.IsoMesh(*K.cut_sphere())
    f, sizes = M.fixture_3d(), M.FIXTURE_3D_SIZES
    np.savez(tmp_path / "in.npz", sizes=np.array(sizes), f=f, **{k: v for k, v in zip(mesh._fields, mesh)})
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "smooth_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"].all()
    _same_mesh([o["taubin_" + k] for k in mesh._fields], fi.smooth_mesh(mesh, 4, boundary="slide", max_move=0.5))
    bare = fi.smooth_mesh(mesh._replace(normals=None, keys=None), 2, mu=0.0)
    assert o["bare_has_normals"][0] == 0
    _same_mesh([o["bare_" + k] for k in ("vertices", "indices", "keys")], [bare.vertices, bare.indices, bare.keys])
    _same_mesh([o["normals_" + k] for k in mesh._fields], fi.mesh_normals(mesh._replace(normals=None)))
    _same_mesh([o["field_" + k] for k in mesh._fields], fi.iso_surface(f, sizes, largest=1, smooth=3))


# ---- every error code -------------------------------------------------------------------------------------------------

def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    INVALID = 1
    v = np.array([[0.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.5, 2.5, 0.5], [0.5, 0.5, 2.5], [7.0, 7.0, 7.0]], np.float32)
    idx = np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    h, out = C.c_void_p(), C.c_void_p()

    def create(vertices):
        vertices = np.ascontiguousarray(vertices, np.float32)
        assert L.fi_mesh_create(C.byref(h), 3, 5, C.c_void_p(vertices.ctypes.data), None, None, 2, C.c_void_p(idx.ctypes.data), _capi.FI_HOST) == 0

    def smooth(mesh=None, **kw):
        o = dict(iterations=2, lam=0.5, mu=-0.53, boundary=0, max_move=0.0, normals=0)
        o.update(kw)
        opt = _capi.FiSmoothOptions(o["iterations"], o["lam"], o["mu"], o["boundary"], o["max_move"], o["normals"])
        out.value = 12345
        return L.fi_mesh_smooth(h if mesh is None else mesh, C.byref(opt), C.byref(out))

    def normals(mesh=None):
        out.value = 12345
        return L.fi_mesh_normals(h if mesh is None else mesh, C.byref(out))

    create(v)
    try:
        nan = float("nan")
        for kw in ({"iterations": -1}, {"lam": -0.25}, {"lam": 1.25}, {"lam": nan}, {"mu": 0.25}, {"mu": -2.5}, {"mu": nan},
                   {"max_move": -1.0}, {"max_move": nan}, {"boundary": -1}, {"boundary": 3}, {"normals": -1}, {"normals": 2}):
            assert smooth(**kw) == INVALID and not out.value and L.fi_last_error(), kw
        out.value = 12345
        assert L.fi_mesh_smooth(h, None, C.byref(out)) == INVALID and not out.value
        opt = _capi.FiSmoothOptions(1, 0.5, 0.0, 0, 0.0, 0)
        assert L.fi_mesh_smooth(h, C.byref(opt), None) == INVALID
        assert L.fi_mesh_normals(h, None) == INVALID
        for kw in ({"lam": 0.0}, {"lam": 1.0}, {"mu": -2.0}, {"mu": -0.0}, {"iterations": 0}, {"boundary": 2, "normals": 1}):
            assert smooth(**kw) == 0 and out.value, kw
            # no normals went in: none come out
            n = np.empty((5, 3), np.float32)
            assert L.fi_mesh_copy(out, None, C.c_void_p(n.ctypes.data), None, None, _capi.FI_HOST) == INVALID
            keys = np.empty(5, np.int64)
            assert L.fi_mesh_copy(out, None, None, None, C.c_void_p(keys.ctypes.data), _capi.FI_HOST) == 0 and keys.tolist() == [0, 1, 2, 3, 4]
            L.fi_mesh_destroy(out)
        assert normals() == 0 and out.value
        n = np.empty((5, 3), np.float32)
        assert L.fi_mesh_copy(out, None, C.c_void_p(n.ctypes.data), None, None, _capi.FI_HOST) == 0 and not n[4].any() and n[:4].any(axis=1).all()
        L.fi_mesh_destroy(out)
    finally:
        L.fi_mesh_destroy(h)
    for bad in (np.nan, np.inf):
        w = v.copy()
        w[2, 1] = bad
        create(w)
        try:
            assert smooth() == INVALID and not out.value and L.fi_last_error()
            assert smooth(iterations=0) == INVALID and not out.value
            assert normals() == INVALID and not out.value
        finally:
            L.fi_mesh_destroy(h)
        w = v.copy()
        w[4, 1] = bad                                                    # (an unused vertex may hold anything)
        create(w)
        try:
            assert smooth() == 0 and out.value
            L.fi_mesh_destroy(out)
            assert normals() == 0 and out.value
            L.fi_mesh_destroy(out)
        finally:
            L.fi_mesh_destroy(h)
    assert smooth(mesh=C.c_void_p()) == INVALID and not out.value
    assert normals(mesh=C.c_void_p()) == INVALID and not out.value
    mesh = fi.IsoMesh(v, None, idx, None)
    with pytest.raises(ValueError):
        fi.smooth_mesh(mesh, boundary="loose")
    with pytest.raises(ValueError):
        fi.smooth_mesh(mesh, normals="average")
