"""Points on a mesh and mesh-to-surface deviation on the device (fi_meshpts.hip through fi_mesh_sample / fi_mesh_deviation,
sample_mesh and mesh_deviation) against the numpy restatement of the contract (tests/meshpts_reference.py): every output array
and every field of the result structs, bit for bit."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_parts_reference as M
import meshpts_reference as P
import simplify_reference as S
import smooth_cases as K

pytestmark = pytest.mark.gpu

SEAMS = (1, 63, 64, 65, 255, 256, 257, 16385)       # a wave, a block, the serial partials of more than one block


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b, what=""):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    bad = np.flatnonzero(_bytes(a).reshape(len(a), -1) != _bytes(b).reshape(len(b), -1)) if len(a) else []
    assert len(bad) == 0, (what, len(bad), bad[:3])


def _mesh(fi, v, idx, normals=None):
    v = np.asarray(v, np.float32)
    return fi.IsoMesh(v, normals, np.asarray(idx, np.int32).reshape(-1, v.shape[1]), None)


def _check_sample(fi, mesh, n, seed=0, what=""):
    """sample_mesh with face normals (and vertex normals where the mesh has them) against the restatement"""
    what = "%s: n %d seed %d" % (what, n, seed)
    modes = ["face"] + (["vertex"] if mesh.normals is not None else [])
    for mode in modes:
        want = P.sample(mesh.vertices, mesh.normals, mesh.indices, n, seed, P.NORMALS[mode])
        got = fi.sample_mesh(mesh, n, seed, normals=mode, primitives=True)
        for g, w, name in zip(got, want, ("positions", "normals", "primitives")):
            _same(g, w, "%s, %s, %s" % (what, mode, name))
    return got


def _same_stats(got, want, what=""):
    for k in ("queries", "counted", "beyond", "invalid", "at"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("max", "mean", "rms"):
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (what, k, got[k], want[k])
    D = len(got["where"])
    assert np.array_equal(_bytes(got["where"]), _bytes(want["where"][:D])), (what, "where")


def _check_deviation(fi, a, b, samples, seed=0, max_distance=np.inf, symmetric=True, what=""):
    got = fi.mesh_deviation(a, b, samples, seed, max_distance, symmetric, vertex_distances=True)
    tops = []
    for name, (x, y) in (("a_to_b", (a, b)), ("b_to_a", (b, a))):
        if name == "b_to_a" and not symmetric:
            assert got[name] is None
            continue
        of_s, of_v, vd = P.deviation(x.vertices, x.indices, y.vertices, y.indices, samples, seed, max_distance)
        _same_stats(got[name]["samples"], of_s, "%s %s samples" % (what, name))
        _same_stats(got[name]["vertices"], of_v, "%s %s vertices" % (what, name))
        _same(got[name]["vertex_distances"], vd, "%s %s vertex distances" % (what, name))
        tops += [of_s["max"], of_v["max"]]
    assert got["hausdorff"] == max(tops), what
    return got


@functools.lru_cache(maxsize=None)
def cube():
    return S.cube_mesh()


@functools.lru_cache(maxsize=None)
def coarse_cube(placement):
    v, t = cube()
    r = S.simplify(v, None, t, 3.0, None, placement)
    return r.vertices, r.indices


# ---- the cases of tests/test_meshpts_reference.py ---------------------------------------------------------------------

def test_cube_samples(fi):
    mesh = _mesh(fi, *cube())
    for n in (1, 255, 256, 257, 5000):
        _check_sample(fi, mesh, n, 7, "cube")
    _check_deviation(fi, mesh, mesh, 5000, 7, symmetric=False, what="cube against itself")


@pytest.mark.parametrize("placement", [S.QUADRIC, S.MEAN])
def test_cube_simplified(fi, placement):
    fine, coarse = _mesh(fi, *cube()), _mesh(fi, *coarse_cube(placement))
    got = _check_deviation(fi, coarse, fine, 4096, 0, what="simplified cube")
    if placement == S.QUADRIC:
        assert got["hausdorff"] < 1e-5
    else:
        assert got["a_to_b"]["samples"]["max"] > 0.5 and got["b_to_a"]["samples"]["max"] > 0.5
    _check_deviation(fi, fine, coarse, 500, 0, 0.25, what="simplified cube, max_distance 0.25")


def test_shifted_copies(fi):
    v, t, _rim = K.flat_grid(6, 3.125)
    got = _check_deviation(fi, _mesh(fi, v, t), _mesh(fi, v + np.array([0, 0, 0.375], np.float32), t), 1000, 3, what="flat grid")
    for side in ("a_to_b", "b_to_a"):
        for r in (got[side]["samples"], got[side]["vertices"]):
            assert r["max"] == r["mean"] == r["rms"] == 0.375 and r["at"] == 0
    v, seg = S.square_polyline()
    _check_sample(fi, _mesh(fi, v, seg), 64, 5, "square")
    _check_deviation(fi, _mesh(fi, v, seg), _mesh(fi, v + np.array([0.25, 0], np.float32), seg), 500, 1, what="square")


def test_constructed_cases(fi):
    cv, ct = cube()
    for name, v, t in K.constructed():
        mesh = _mesh(fi, v, t)
        other = _mesh(fi, cv[:, :mesh.vertices.shape[1]] * np.float32(0.25), ct[:40, :mesh.vertices.shape[1]])
        if P.integer_weights(mesh.vertices, mesh.indices)[2] == 0:
            with pytest.raises(fi.FiError) as e:
                fi.sample_mesh(mesh, 10)
            assert e.value.code == 1, name
        else:
            for n in (1, 300):
                _check_sample(fi, mesh, n, 2, name)
        got = _check_deviation(fi, mesh, other, 300, 2, what=name)
        got = _check_deviation(fi, mesh, mesh, 300, 2, symmetric=False, what=name + " against itself")
        # a vertex against its own primitives: the closest point is a + t ab in fp32, a few roundings at coordinates below 4
        assert got["a_to_b"]["vertices"]["max"] <= 4 * float(np.spacing(np.float32(4.0)))
    v, t = cube()
    w = v.copy()
    w[t[5, 1], 2] = np.nan
    got = _check_deviation(fi, _mesh(fi, w, t), _mesh(fi, v, t), 500, 0, what="a non-finite vertex")
    assert got["a_to_b"]["vertices"]["invalid"] == 1


def test_vertex_normals_that_have_no_direction(fi):
    """a zero or non-finite length of the interpolated vertex normal gives the face normal: all zeros, all NaN, and a mix in
    which some primitives interpolate and some fall back"""
    v, t = cube()
    face = fi.sample_mesh(_mesh(fi, v, t), 2000, 9, normals="face")[1]
    mixed = ((v - np.float32(6.75)) / np.linalg.norm(v - np.float32(6.75), axis=1, keepdims=True)).astype(np.float32)
    mixed[::3] = 0.0
    mixed[1::7] = np.nan
    mixed[5::11] = np.inf
    for name, nrm in (("zeros", np.zeros_like(v)), ("NaN", np.full_like(v, np.nan)), ("mixed", mixed)):
        got = _check_sample(fi, _mesh(fi, v, t, nrm), 2000, 9, "cube, vertex normals: " + name)
        if name != "mixed":
            _same(got[1], face, name)
        else:
            assert np.isfinite(got[1]).all() and not np.array_equal(got[1], face)


# ---- the fixtures through both extractors, both normals modes -------------------------------------------------------------

FIELDS = {"sphere": (lambda: S.sphere_field()[0], [24, 24, 24]), "3d": (M.fixture_3d, M.FIXTURE_3D_SIZES),
          "2d": (M.fixture_2d, M.FIXTURE_2D_SIZES)}


@pytest.mark.parametrize("method", ["iso", "dual"])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_extracted_meshes(fi, name, method):
    make, sizes = FIELDS[name]
    mesh = (fi.iso_surface if method == "iso" else fi.dual_contour)(make(), sizes)
    assert len(mesh.indices) > 100 and mesh.normals is not None
    what = "%s %s" % (name, method)
    pos, nrm, _prim = _check_sample(fi, mesh, 3001, 4, what)
    # vertex normals interpolated over an extracted surface stay close to its face normals
    face = fi.sample_mesh(mesh, 3001, 4, normals="face")[1]
    assert (nrm.astype(np.float64) * face).sum(axis=1).mean() > 0.9
    coarse = fi.simplify_mesh(mesh, 2.0)                  # (few primitives: the restatement's brute force stays quick)
    _check_deviation(fi, mesh, coarse, 700, 4, symmetric=False, what=what)


# ---- the seams: a wave, a block, the serial partials ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def strip(ndim, nv):
    """nv vertices along a noisy line, joined into a triangle strip (2-D: a polyline); one vertex: a primitive that names it
    ndim times (it is used, and there is nothing to sample)"""
    rng = np.random.default_rng(100 * ndim + nv)
    v = (rng.normal(size=(nv, ndim)) * 0.3).astype(np.float32)
    v[:, 0] += np.arange(nv, dtype=np.float32) * np.float32(0.5)
    if nv < ndim:
        return v, np.zeros((1, ndim), np.int32)
    return v, (np.arange(nv - ndim + 1)[:, None] + np.arange(ndim)[None, :]).astype(np.int32)


@pytest.mark.parametrize("ndim", [3, 2])
def test_seams(fi, ndim):
    cv, ct = cube()
    other = _mesh(fi, cv[:, :ndim], ct[:24, :ndim])
    long = _mesh(fi, *strip(ndim, 300))
    for n in SEAMS:
        _check_sample(fi, long, n, n, "%d-D strip" % ndim)
        v, idx = strip(ndim, n)
        mesh = _mesh(fi, v, idx)
        got = _check_deviation(fi, mesh, other, n, 1, symmetric=False, what="%d-D, %d vertices" % (ndim, n))
        assert got["a_to_b"]["vertices"]["queries"] == n
        assert got["a_to_b"]["samples"]["queries"] == (n if n >= ndim else 0)


def test_one_primitive(fi):
    for v, idx in (([[1, 1, 1], [4, 1, 2], [2, 5, 1.5]], [[0, 1, 2]]), ([[1, 1], [4, 2.5]], [[0, 1]])):
        mesh = _mesh(fi, v, idx)
        for n in (1, 1000):
            got = _check_sample(fi, mesh, n, 3, "one primitive")
            assert not got[2].any()
        _check_deviation(fi, mesh, _mesh(fi, np.asarray(v, np.float32) + np.float32(1.0), idx), 1000, 3, what="one primitive")


@pytest.fixture(scope="module")
def large(fi):
    f, _c = S.sphere_field(96, 44.0)
    mesh = fi.iso_surface(f, [96, 96, 96])
    assert (len(mesh.vertices), len(mesh.indices)) == (36520, 73036)
    return mesh


def test_large_sphere_a_million_samples(fi, large):
    """sampling alone: a brute-force distance of a million points would take the restatement minutes"""
    n = 1000003
    got = _check_sample(fi, large, n, 11, "96^3")
    assert np.all(np.diff(got[2]) >= 0) and got[2][-1] > 73000
    a, b = fi.sample_mesh(large, 4099, 1, normals=None), fi.sample_mesh(large, 4099, 2, normals=None)
    assert a.shape == b.shape == (4099, 3) and not np.array_equal(a, b)                # two seeds differ
    _same(fi.sample_mesh(large, 4099, 2 ** 64 - 1, normals=None), P.sample(large.vertices, None, large.indices, 4099, 2 ** 64 - 1)[0], "seed 2^64 - 1")


# ---- what the unit is for -------------------------------------------------------------------------------------------------

def test_deviation_of_simplified_and_smoothed_meshes(fi):
    f, _c = S.sphere_field()
    mesh = fi.iso_surface(f, [24, 24, 24])
    coarse = fi.simplify_mesh(mesh, 3.0)
    faired = fi.smooth_mesh(mesh, 5)
    got = _check_deviation(fi, coarse, mesh, 1500, 0, what="simplified sphere")
    assert 0.0 < got["hausdorff"] < 1.0
    got = _check_deviation(fi, faired, mesh, 1500, 0, what="smoothed sphere")
    assert 0.0 < got["hausdorff"] < 0.5
    index = fi.SurfaceIndex.from_mesh(mesh)
    one = fi.mesh_deviation(faired, index, 1500, symmetric=False)
    _same_stats(one["a_to_b"]["samples"], got["a_to_b"]["samples"], "a SurfaceIndex")
    _same_stats(one["a_to_b"]["vertices"], got["a_to_b"]["vertices"], "a SurfaceIndex")
    assert one["b_to_a"] is None and "vertex_distances" not in one["a_to_b"]
    with pytest.raises(ValueError):
        fi.mesh_deviation(faired, index, 1500)
    with pytest.raises(ValueError):
        fi.mesh_deviation(faired, fi.SurfaceIndex.from_mesh(_mesh(fi, *S.square_polyline())), 10, symmetric=False)


def test_repeated_calls_return_the_same_bytes(fi, large):
    f, _c = S.sphere_field()
    small = fi.iso_surface(f, [24, 24, 24])

    def run():
        s = fi.sample_mesh(large, 70001, 5, normals="vertex", primitives=True)
        d = fi.mesh_deviation(small, large, 20000, 5, vertex_distances=True)
        return s, d

    def same(x, y):
        for u, w in zip(x[0], y[0]):
            _same(u, w, "samples")
        for side in ("a_to_b", "b_to_a"):
            _same_stats(x[1][side]["samples"], y[1][side]["samples"], side)
            _same_stats(x[1][side]["vertices"], y[1][side]["vertices"], side)
            _same(x[1][side]["vertex_distances"], y[1][side]["vertex_distances"], side)

    first = run()
    same(first, run())
    fi.smooth_mesh(large, 2)                                                   # (the arena is shared: other units in between)
    fi.simplify_mesh(large, 2.0)
    same(first, run())


# ---- the Python keywords ----------------------------------------------------------------------------------------------

def test_python_keywords(fi):
    mesh = _mesh(fi, *cube())
    pos = fi.sample_mesh(mesh, 100)
    assert isinstance(pos, tuple) and len(pos) == 2                           # normals="face" is the default
    only = fi.sample_mesh(mesh, 100, normals=None)
    assert isinstance(only, np.ndarray) and only.shape == (100, 3) and np.array_equal(only, pos[0])
    p, prim = fi.sample_mesh(mesh, 100, seed=0, normals=None, primitives=True)
    assert prim.dtype == np.int64 and prim.shape == (100,)
    assert [a.shape for a in fi.sample_mesh(mesh, 0, primitives=True)] == [(0, 3), (0, 3), (0,)]
    with pytest.raises(ValueError):
        fi.sample_mesh(mesh, 10, normals="smooth")
    with pytest.raises(ValueError):
        fi.sample_mesh(mesh, -1)
    with pytest.raises(fi.FiError):
        fi.sample_mesh(mesh, 10, normals="vertex")                            # the mesh has no normals
    coarse = _mesh(fi, *coarse_cube(S.MEAN))
    d = fi.mesh_deviation(coarse, mesh)
    assert d["a_to_b"]["samples"]["queries"] == d["b_to_a"]["samples"]["queries"] == 100000
    assert "vertex_distances" not in d["a_to_b"] and d["hausdorff"] > 0.5
    d = fi.mesh_deviation(coarse, mesh, samples=0, symmetric=False, vertex_distances=True)
    assert d["a_to_b"]["samples"]["queries"] == 0 and d["a_to_b"]["samples"]["at"] == -1 and d["b_to_a"] is None
    assert d["a_to_b"]["vertex_distances"].shape == (56,) and d["hausdorff"] == d["a_to_b"]["vertices"]["max"]
    with pytest.raises(ValueError):
        fi.mesh_deviation(coarse, mesh, samples=-1)
    with pytest.raises(ValueError):
        fi.mesh_deviation(coarse, _mesh(fi, *S.square_polyline()))
    with pytest.raises(fi.FiError):
        fi.mesh_deviation(coarse, mesh, max_distance=-1.0)


def test_device_pointers(fi, tmp_path):
    """torch device tensors in and out (a fresh process, tests/meshpts_torch_worker.py: torch stays out of this one): the host
    path's answers"""
    f, _c = S.sphere_field()
    mesh = fi.iso_surface(f, [24, 24, 24])
    cv, ct = cube()
    np.savez(tmp_path / "in.npz", cube_vertices=cv * np.float32(1.5), cube_indices=ct, **{k: v for k, v in zip(mesh._fields, mesh)})
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "meshpts_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"].all()
    want = fi.sample_mesh(mesh, 5000, 3, normals="vertex", primitives=True)
    for k, w in zip(("positions", "normals", "primitives"), want):
        _same(o["sample_" + k], w, k)
    _same(o["bare_positions"], fi.sample_mesh(mesh._replace(normals=None, keys=None), 777, 1, normals=None), "bare")
    other = fi.IsoMesh(cv * np.float32(1.5), None, ct, None)
    d = fi.mesh_deviation(mesh, other, 3000, 2, vertex_distances=True)
    for side in ("a_to_b", "b_to_a"):
        for what in ("samples", "vertices"):
            got = {k: o["%s_%s_%s" % (side, what, k)] for k in d[side][what]}
            got = {k: (v if k == "where" else v[()]) for k, v in got.items()}
            _same_stats(got, d[side][what], side + " " + what)
        _same(o[side + "_vertex_distances"], d[side]["vertex_distances"], side)


# ---- every error code -------------------------------------------------------------------------------------------------

def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    INVALID, UNSUPPORTED = 1, 5
    v = np.array([[0.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.5, 2.5, 0.5], [0.5, 0.5, 2.5], [7.0, 7.0, 7.0]], np.float32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (5, 1))
    idx = np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def create(vertices, normals, indices):
        h = C.c_void_p()
        vertices = np.ascontiguousarray(vertices, np.float32)
        indices = np.ascontiguousarray(indices, np.int32)
        assert L.fi_mesh_create(C.byref(h), vertices.shape[1], len(vertices), ptr(vertices), None if normals is None else ptr(normals), None,
                                len(indices), ptr(indices) if len(indices) else None, _capi.FI_HOST) == 0
        return h

    bare, full = create(v, None, idx), create(v, nrm, idx)
    flat = create(np.array([[1, 1, 1], [2, 1, 1], [3, 1, 1]], np.float32), None, [[0, 1, 2]])
    empty = create(v, None, np.zeros((0, 3), np.int32))
    line = create(v[:, :2], None, idx[:, :2])
    surf, surf2 = C.c_void_p(), C.c_void_p()
    assert L.fi_surface_from_mesh(C.byref(surf), bare) == 0 and L.fi_surface_from_mesh(C.byref(surf2), line) == 0
    pos = np.full((8, 3), 77.0, np.float32)
    out_n = np.full((8, 3), 77.0, np.float32)
    prim = np.full(8, 77, np.int64)
    H = _capi.FI_HOST
    try:
        def sample(mesh=bare, n=8, mode=0, positions=pos, normals=out_n, primitives=prim, memory=H):
            return L.fi_mesh_sample(mesh, n, 1, mode, None if positions is None else ptr(positions), None if normals is None else ptr(normals),
                                    None if primitives is None else ptr(primitives), memory)

        assert sample(mesh=None) == INVALID and L.fi_last_error()
        assert sample(n=-1) == INVALID
        assert sample(positions=None) == INVALID
        for mode in (-1, 2):
            assert sample(mode=mode) == INVALID
        for memory in (-1, 2):
            assert sample(memory=memory) == INVALID
        assert sample(mode=1) == INVALID                                        # vertex normals of a mesh without normals
        assert sample(mesh=flat) == INVALID and sample(mesh=empty) == INVALID   # nothing of positive measure; no primitives
        assert sample(n=2 ** 31) == UNSUPPORTED
        assert (pos == 77.0).all() and (out_n == 77.0).all() and (prim == 77).all()
        assert sample(n=0) == 0 and sample(n=0, positions=None, mesh=empty) == 0
        assert (pos == 77.0).all() and (out_n == 77.0).all() and (prim == 77).all()   # n = 0 writes nothing
        assert sample(mode=1, normals=None) == 0 and sample(mesh=full, mode=1) == 0
        assert sample(normals=None, primitives=None) == 0 and (pos != 77.0).all()

        s, w = _capi.FiDeviation(), _capi.FiDeviation()
        vd = np.empty(5, np.float32)

        def deviation(a=bare, b=surf, samples=10, max_distance=np.inf, of_s=s, of_v=w, distances=vd, memory=H):
            return L.fi_mesh_deviation(a, b, samples, 1, max_distance, None if of_s is None else C.byref(of_s),
                                       None if of_v is None else C.byref(of_v), None if distances is None else ptr(distances), memory)

        assert deviation(a=None) == INVALID and deviation(b=None) == INVALID and L.fi_last_error()
        assert deviation(of_s=None, of_v=None, distances=None) == INVALID
        assert deviation(b=surf2) == INVALID and deviation(a=line) == INVALID   # 3-D against 2-D
        assert deviation(samples=-1) == INVALID
        for bad in (np.nan, -0.5):
            assert deviation(max_distance=bad) == INVALID
        for memory in (-1, 2):
            assert deviation(memory=memory) == INVALID
        assert deviation(samples=2 ** 31) == UNSUPPORTED
        assert deviation() == 0 and s.queries == 10 and w.queries == 4 and np.isnan(vd[4]) and not vd[:4].any()
        assert deviation(of_s=None, of_v=None) == 0 and deviation(of_v=None, distances=None) == 0
        assert deviation(a=flat) == 0 and (s.queries, s.at, s.max) == (0, -1, 0.0) and w.queries == 3
        assert deviation(a=empty) == 0 and (s.queries, w.queries, w.at) == (0, 0, -1) and np.isnan(vd).all()
        assert deviation(max_distance=0.0) == 0 and s.counted + s.beyond == 10
    finally:
        for h in (surf, surf2):
            L.fi_surface_destroy(h)
        for h in (bare, full, flat, empty, line):
            L.fi_mesh_destroy(h)
