"""Rigid registration on the device (fi_register.hip through fi_mesh_register / fi_points_register, register_points and
LatticeField.register) against the numpy restatement of the contract (tests/register_reference.py): every field of
fi_registration, the transformed points and the distances, bit for bit."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import register_reference as G
import simplify_reference as S

pytestmark = pytest.mark.gpu

SEAMS = (1, 63, 64, 65, 255, 256, 257, 16385)       # a wave, a block, the ordered partials of more than one block
INTS = ("iterations", "converged", "fixed_mask", "queries", "counted", "beyond", "invalid", "degenerate")
REALS = ("rms", "weighted_rms", "last_rotation", "last_translation")


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want, what=""):
    """every field of the result, the transformed points and the distances"""
    for k in INTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in REALS:
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (what, k, got[k], want[k])
    assert got["transform"].dtype == np.float64 and got["transform"].shape == want["transform"].shape, what
    assert np.array_equal(_bytes(got["transform"]), _bytes(want["transform"])), (what, got["transform"], want["transform"])
    for k in ("transformed", "distances"):
        if k in got:
            assert got[k].dtype == np.float32 and got[k].shape == want[k].shape, (what, k)
            # (a NaN's sign and payload are no part of the contract: 0 * inf is -NaN on one machine and +NaN on another)
            g, w = np.asarray(got[k]).copy(), np.asarray(want[k]).copy()
            both = np.isnan(g) & np.isnan(w)
            g[both], w[both] = 0, 0
            assert np.array_equal(_bytes(g), _bytes(w)), (what, k)


def _mesh(fi, v, idx):
    v = np.asarray(v, np.float32)
    return fi.IsoMesh(v, None, np.asarray(idx, np.int32).reshape(-1, v.shape[1]), None)


def _check(fi, target, source, what="", normals=None, **kw):
    """register_points against the restatement; target: (vertices, indices) of a mesh or an (m, D) array of points"""
    ref = dict(kw)
    ref["mode"] = G.MODES[ref.pop("mode", "plane")]
    ref["loss"] = G.LOSSES[ref.pop("loss", None)]
    if isinstance(target, tuple):
        want = G.register(G.Target(*target), source, **ref)
        got = fi.register_points(source, _mesh(fi, *target), transformed=True, distances=True, **kw)
    else:
        want = G.register(G.Target(points=target, normals=normals), source, **ref)
        got = fi.register_points(source, target, normals, transformed=True, distances=True, **kw)
    _same(got, want, what)
    return got


@functools.lru_cache(maxsize=None)
def cube():
    return G.cube_case()


@functools.lru_cache(maxsize=None)
def rectangle():
    return G.rectangle_case()


@functools.lru_cache(maxsize=None)
def many(n):
    """n sample points of the cube, turned 3 degrees and shifted"""
    return G.cube_case(n, 3.0, 11)


# ---- the cases of tests/test_register_reference.py -----------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["plane", "point"])
def test_cube(fi, mode):
    v, t, _pts, _nrm, src, (R, tt) = cube()
    got = _check(fi, (v, t), src, "cube " + mode, mode=mode, max_iterations=8)
    if mode == "plane":
        assert got["converged"] == 1 and np.abs(got["transform"][:3, :3] - R).max() < 1e-6
        assert np.abs(got["transform"][:3, 3] - tt).max() < 1e-5


@pytest.mark.parametrize("mode", ["plane", "point"])
def test_rectangle(fi, mode):
    v, s, _on, _nrm, src, _truth = rectangle()
    got = _check(fi, (v, s), src, "rectangle " + mode, mode=mode, max_iterations=6)
    assert got["transform"].shape == (3, 3)


@pytest.mark.parametrize("mode,normals", [("plane", True), ("point", True), ("point", False)])
def test_point_set_targets(fi, mode, normals):
    for case, what in ((cube(), "cube"), (rectangle(), "rectangle")):
        _v, _t, pts, nrm, src, _truth = case
        _check(fi, pts, src, "%s points %s" % (what, mode), normals=nrm if normals else None, mode=mode, max_iterations=5)


@pytest.mark.parametrize("n", SEAMS)
def test_seams(fi, n):
    v, t, pts, nrm, src, _truth = many(n)
    its = 2 if n > 1000 else 3
    _check(fi, (v, t), src, "cube n %d" % n, max_iterations=its)
    _check(fi, (v, t), src, "cube n %d point" % n, mode="point", max_iterations=1)
    if n <= 1000:
        _check(fi, pts, src, "set n %d" % n, normals=nrm, max_iterations=2)
    rv, rs, ron, rnrm, rsrc, _truth = G.rectangle_case(n, 4.0, 2)
    _check(fi, (rv, rs), rsrc, "rectangle n %d" % n, max_iterations=2)


@pytest.mark.parametrize("loss", ["huber", "cauchy", "tukey"])
def test_losses(fi, loss):
    v, t, src, (R, _tt) = G.outlier_case()
    got = _check(fi, (v, t), src, loss, max_iterations=8, max_distance=1.5, loss=loss, scale=0.1)
    if loss == "tukey":
        assert np.abs(got["transform"][:3, :3] - R).max() < 1e-6
    _check(fi, (v, t), src, loss + " tuned, point", mode="point", max_iterations=2, loss=loss, scale=0.25, tuning=2.0)
    rv, rs, _on, _nrm, rsrc, _truth = rectangle()
    _check(fi, (rv, rs), rsrc, loss + " 2-D", max_iterations=3, loss=loss, scale=0.05)


def test_max_distance(fi):
    v, t, _pts, _nrm, src, _truth = cube()
    got = _check(fi, (v, t), src, "some rejected at the start", max_iterations=0, max_distance=0.5)
    assert 0 < got["beyond"] < 600 and got["counted"] + got["beyond"] == 600
    _check(fi, (v, t), src, "some rejected", max_iterations=4, max_distance=0.5)
    got = _check(fi, (v, t), src, "all rejected", max_iterations=4, max_distance=0.0)
    assert got["counted"] == 0 and got["beyond"] == 600 and got["iterations"] == 0
    assert np.array_equal(got["transform"], np.eye(4)) and np.isinf(got["distances"]).all()


def test_initial_and_no_iterations(fi):
    v, t, _pts, _nrm, src, (R, tt) = cube()
    start = np.eye(4)
    start[:3, :3], start[:3, 3] = G.rotation((1, 2, 3), -6.0), tt * 0.9
    start[3] = (5.0, 6.0, 7.0, 8.0)                                            # the last row is ignored
    got = _check(fi, (v, t), src, "initial", max_iterations=4, initial=start)
    assert np.array_equal(got["transform"][3], (0.0, 0.0, 0.0, 1.0))
    got = _check(fi, (v, t), src, "evaluation alone", max_iterations=0, initial=start)
    assert got["iterations"] == 0 and np.array_equal(got["transform"][:3], start[:3])
    got = _check(fi, (v, t), src, "evaluation alone, identity", mode="point", max_iterations=0)
    assert np.array_equal(_bytes(got["transformed"]), _bytes(src))


def test_flat_grid_fixes_what_it_cannot_see(fi):
    v, t, src = G.flat_case()
    got = _check(fi, (v, t), src, "flat grid", max_iterations=6)
    assert got["fixed_mask"] == 0b011100 and got["converged"] == 1


def test_non_finite_points(fi):
    v, t, _pts, _nrm, src, _truth = cube()
    src = src.copy()
    src[5, 1], src[77, 0], src[300] = np.nan, np.inf, -np.inf
    got = _check(fi, (v, t), src, "non-finite source", max_iterations=3)
    assert got["invalid"] == 3
    got = _check(fi, (v, t), np.full((70, 3), np.nan, np.float32), "nothing finite", max_iterations=3)
    assert got["invalid"] == 70 and got["iterations"] == 0
    v = v.copy()
    v[[3, 400]] = np.nan                                                       # their triangles are never nearest
    _check(fi, (v, t), src, "non-finite target vertices", max_iterations=3)
    _v, _t, pts, nrm, src, _truth = cube()
    pts, nrm = pts.copy(), nrm.copy()
    pts[10, 2] = np.inf
    nrm[20], nrm[30, 0] = 0.0, np.nan                                          # degenerate pairs
    got = _check(fi, pts, src, "non-finite target points", normals=nrm, max_iterations=3)
    assert got["degenerate"] > 0


def test_degenerate_triangles(fi):
    v, t, _pts, _nrm, src, _truth = cube()
    flat = np.array([[20, 20, 20], [21, 20, 20], [22, 20, 20]], np.float32)
    v2 = np.concatenate([v, flat])
    t2 = np.concatenate([t, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)
    src = np.concatenate([src, [[20.5, 20.1, 20.0], [21.5, 19.9, 20.0]]]).astype(np.float32)
    got = _check(fi, (v2, t2), src, "zero-area triangle, plane", max_iterations=0)
    assert got["degenerate"] == 2 and got["counted"] == 600
    got = _check(fi, (v2, t2), src, "zero-area triangle, point", mode="point", max_iterations=0)
    assert got["degenerate"] == 0 and got["counted"] == 602


def test_prebuilt_index_and_repeats(fi):
    from field_interpolation_amd import _capi
    from field_interpolation_amd.api import _mesh_handle, _register_options, _register_to_mesh
    v, t, _pts, _nrm, src, _truth = cube()
    mesh = _mesh(fi, v, t)
    first = fi.register_points(src, mesh, max_iterations=4, transformed=True, distances=True)
    L = _capi.lib()
    h = _mesh_handle(mesh)[0]
    surf = C.c_void_p()
    assert L.fi_surface_from_mesh(C.byref(surf), h) == 0
    try:
        opt = _register_options("plane", 4, np.inf, 1e-6, 1e-6, None, 0.0, 0.0)
        _same(_register_to_mesh(h, surf, 3, src, opt, None, True, True), first, "a prebuilt index")
    finally:
        L.fi_surface_destroy(surf)
        L.fi_mesh_destroy(h)
    _same(fi.register_points(src, mesh, max_iterations=4, transformed=True, distances=True), first, "a second call")
    fi.smooth_mesh(mesh, 2)                                                    # (the arena is shared: other units in between)
    fi.sample_mesh(mesh, 1000)
    _same(fi.register_points(src, mesh, max_iterations=4, transformed=True, distances=True), first, "a third call")
    index = fi.SurfaceIndex.from_mesh(mesh)
    point = fi.register_points(src, mesh, mode="point", max_iterations=3, transformed=True, distances=True)
    _same(fi.register_points(src, index, mode="point", max_iterations=3, transformed=True, distances=True), point, "a SurfaceIndex")
    with pytest.raises(ValueError):
        fi.register_points(src, index)
    _v, _t, pts, nrm, src, _truth = cube()
    one = fi.register_points(src, pts, nrm, max_iterations=3, transformed=True)
    _same(fi.register_points(src, fi.PointIndex(pts), nrm, max_iterations=3, transformed=True), one, "a PointIndex")


def test_python_keywords(fi):
    v, t, _pts, _nrm, src, (R, tt) = cube()
    mesh = _mesh(fi, v, t)
    got = fi.register_points(src, mesh)
    assert "transformed" not in got and "distances" not in got and got["converged"] == 1 and got["iterations"] <= 8
    moved = fi.apply_transform(got["transform"], src)
    assert moved.dtype == np.float64
    assert np.abs(moved - fi.register_points(src, mesh, transformed=True)["transformed"]).max() < 1e-5
    moved, turned = fi.apply_transform(got["transform"], src, np.eye(3))
    assert np.allclose(turned, got["transform"][:3, :3].T)
    empty = fi.register_points(np.zeros((0, 3), np.float32), mesh, transformed=True, distances=True)
    assert empty["queries"] == 0 and np.array_equal(empty["transform"], np.eye(4)) and empty["transformed"].shape == (0, 3)
    for bad in (dict(mode="planes"), dict(loss="l1"), dict(initial=np.eye(3))):
        with pytest.raises(ValueError):
            fi.register_points(src, mesh, **bad)
    with pytest.raises(ValueError):
        fi.register_points(src[:, :2], mesh)
    with pytest.raises(ValueError):
        fi.register_points(src, src)                                           # plane mode on points without normals
    with pytest.raises(fi.FiError):
        fi.register_points(src, mesh, loss="tukey")                            # a loss needs a scale


def test_lattice_field_register(fi):
    """LatticeField.register on a small solved field equals register_points on its extracted mesh"""
    n = 20
    rng = np.random.default_rng(2)
    d = rng.normal(size=(400, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    centre = np.array([9.6, 9.4, 9.5])
    pts = (centre + d * np.array([6.0, 5.0, 4.0])).astype(np.float32)
    nrm = d / np.array([6.0, 5.0, 4.0])
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
    field = fi.sdf_from_points([n, n, n], fi.Weights(), pts, nrm)
    field.assemble()
    assert field.solve_cg(None, 300, 1e-5) is not None
    src = G.moved(pts, G.rotation((3, 1, 2), 4.0), (0.3, 0.2, -0.25))
    for method, mesh in (("iso", field.iso_surface()), ("dual", field.dual_contour())):
        got = field.register(src, method=method, max_iterations=5, transformed=True, distances=True)
        _same(got, fi.register_points(src, mesh, max_iterations=5, transformed=True, distances=True), method)
        assert got["counted"] == 400 and got["iterations"] > 0


def test_device_pointers(fi, tmp_path):
    """torch device tensors in and out (a fresh process, tests/register_torch_worker.py: torch stays out of this one): the host
    path's answers"""
    v, t, pts, nrm, src, _truth = cube()
    np.savez(tmp_path / "in.npz", vertices=v, indices=t, points=pts, normals=nrm, source=src)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "register_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"].all()
    mesh = _mesh(fi, v, t)
    for name, want in (("mesh", fi.register_points(src, mesh, max_iterations=4, transformed=True, distances=True)),
                       ("set", fi.register_points(src, pts, nrm, max_iterations=4, transformed=True, distances=True)),
                       ("point", fi.register_points(src, pts, mode="point", max_iterations=2, transformed=True, distances=True))):
        got = {k: o["%s_%s" % (name, k)] for k in want}
        got = {k: (x if x.ndim else x[()]) for k, x in got.items()}
        _same(got, want, name)


# ---- every error code -------------------------------------------------------------------------------------------------

def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    INVALID, UNSUPPORTED = 1, 5
    H = _capi.FI_HOST
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    v = np.array([[0.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.5, 2.5, 0.5], [0.5, 0.5, 2.5]], np.float32)
    idx = np.array([[0, 1, 2], [1, 2, 3]], np.int32)

    def create(vertices, indices):
        h = C.c_void_p()
        vertices, indices = np.ascontiguousarray(vertices, np.float32), np.ascontiguousarray(indices, np.int32)
        assert L.fi_mesh_create(C.byref(h), vertices.shape[1], len(vertices), ptr(vertices), None, None, len(indices), ptr(indices), H) == 0
        return h

    def points(p):
        h = C.c_void_p()
        p = np.ascontiguousarray(p, np.float32)
        assert L.fi_points_create(C.byref(h), p.shape[1], len(p), ptr(p), H) == 0
        return h

    mesh, line, one = create(v, idx), create(v[:, :2], idx[:, :2]), create(v, idx[:1])
    surf, surf2, surf1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.fi_surface_from_mesh(C.byref(surf), mesh) == 0 and L.fi_surface_from_mesh(C.byref(surf2), line) == 0
    assert L.fi_surface_from_mesh(C.byref(surf1), one) == 0
    cloud, cloud1 = points(v), points(v[:, :1])
    src = np.array([[0.6, 0.7, 0.5], [1.0, 1.0, 0.6], [2.0, 0.7, 0.4]], np.float32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (4, 1))
    res = _capi.FiRegistration()
    moved, dist = np.full((3, 3), 77.0, np.float32), np.full(3, 77.0, np.float32)

    def options(mode=0, max_iterations=2, max_distance=np.inf, rtol=1e-6, ttol=1e-6, loss=-1, tuning=0.0, scale=0.0):
        return _capi.FiRegisterOptions(mode, max_iterations, max_distance, rtol, ttol, loss, tuning, scale)

    def to_mesh(target=mesh, index=None, n=3, source=src, opt=options(), initial=None, out=res, memory=H):
        init = None if initial is None else initial.ctypes.data_as(C.POINTER(C.c_double))
        return L.fi_mesh_register(target, index, n, None if source is None else ptr(source), None if opt is None else C.byref(opt), init,
                                  None if out is None else C.byref(out), ptr(moved), ptr(dist), memory)

    def to_points(target=cloud, normals=nrm, n=3, source=src, opt=options(), out=res, memory=H):
        return L.fi_points_register(target, None if normals is None else ptr(normals), n, None if source is None else ptr(source),
                                    C.byref(opt), None, None if out is None else C.byref(out), ptr(moved), ptr(dist), memory)

    try:
        assert to_mesh(target=None) == INVALID and L.fi_last_error()
        assert to_mesh(target=None, index=surf) == INVALID                      # plane mode on a surface alone
        assert to_points(target=None) == INVALID
        assert to_mesh(source=None) == INVALID and to_points(source=None) == INVALID
        assert to_mesh(out=None) == INVALID and to_points(out=None) == INVALID
        assert to_mesh(opt=None) == INVALID
        assert to_mesh(n=-1) == INVALID
        assert to_mesh(index=surf2) == INVALID and to_mesh(index=surf1) == INVALID   # another dimension; another mesh
        assert to_points(target=cloud1) == INVALID                              # 1-D
        assert to_mesh(opt=options(max_iterations=-1)) == INVALID
        for bad in (np.nan, -0.5):
            assert to_mesh(opt=options(max_distance=bad)) == INVALID
            assert to_mesh(opt=options(rtol=bad)) == INVALID and to_points(opt=options(ttol=bad)) == INVALID
            assert to_mesh(opt=options(loss=2, scale=0.1, tuning=bad)) == INVALID
        for mode in (-1, 2):
            assert to_mesh(opt=options(mode=mode)) == INVALID
        for loss in (-2, 3):
            assert to_mesh(opt=options(loss=loss, scale=1.0)) == INVALID
        for scale in (0.0, -1.0, np.nan):
            assert to_mesh(opt=options(loss=0, scale=scale)) == INVALID
        for memory in (-1, 2):
            assert to_mesh(memory=memory) == INVALID and to_points(memory=memory) == INVALID
        for bad in (np.nan, np.inf):
            start = np.eye(4)
            start[1, 3] = bad
            assert to_mesh(initial=start) == INVALID
        assert to_points(normals=None) == INVALID                              # plane mode without normals
        assert to_mesh(n=2 ** 31) == UNSUPPORTED and to_points(n=2 ** 31) == UNSUPPORTED
        assert (moved == 77.0).all() and (dist == 77.0).all()
        start = np.eye(4)
        start[3] = np.nan                                                      # the last row is ignored
        start[0, 3] = 0.25
        assert to_mesh(n=0, source=None, initial=start) == 0 and res.queries == 0 and res.iterations == 0
        assert list(res.transform) == [1, 0, 0, 0.25, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
        assert (moved == 77.0).all() and (dist == 77.0).all()                   # n = 0 writes nothing
        assert to_mesh() == 0 and res.queries == 3 and res.counted == 3
        assert to_mesh(index=surf) == 0 and to_mesh(target=None, index=surf, opt=options(mode=1)) == 0
        assert to_points() == 0 and to_points(normals=None, opt=options(mode=1)) == 0 and res.counted == 3
        assert (moved != 77.0).all() and (dist != 77.0).all()
    finally:
        for h in (surf, surf2, surf1):
            L.fi_surface_destroy(h)
        for h in (mesh, line, one):
            L.fi_mesh_destroy(h)
        for h in (cloud, cloud1):
            L.fi_points_destroy(h)
