"""Rays and images of lattice fields and depth volumes on the device (fi_march.hip through fi_field_raycast, fi_field_render,
fi_raycast_field, fi_render_field, fi_volume_raycast, fi_volume_render) against the numpy definition of the contract
(tests/march_reference.py): every output array as bit patterns (a NaN matches a NaN).  Closed and open fields at [9, 7, 8],
[12, 11, 10] and 24^3 and a [31, 17] 2-D field; 0, 1, 63, 64, 65 and 257 rays; every lattice point along the 6 axis
directions; 4 096 random rays; rays that are none; steps, refinements, sides, iso, weights with holes, windows, each output
left out, host against device buffers, an FI_F64 context, every error code; images of 1 x 1, 7 x 9, 8 x 8 and 65 x 17 in both
kinds; volumes; the cross-checks against the depth unit and the mesh raycast; tracking; device tensors in a fresh process."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_reference as dref
import march_cases as cases
import march_reference as ref
import ray_cases as RC

pytestmark = pytest.mark.gpu

F = np.float32
SIDES = {ref.FRONT: "front", ref.BACK: "back", ref.EITHER: "either"}


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1 and _capi.FI_MARCH_MAX_SAMPLES == ref.MAX_SAMPLES
    return fi


def _bits_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.dtype == np.float32:
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    else:
        same = got == want
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:5].tolist(), got[~same][:5], want[~same][:5])


def _camera(fi, c):
    return fi.Camera(c.pose, c.fx, c.fy, c.cx, c.cy, c.width, c.height, "z" if c.kind == dref.Z else "range")


def _field(kind, sizes):
    if kind == "open":                       # a smooth field that the box cuts: crossings on the faces, many sheets
        f = RC.smooth(sizes, sum(sizes))
        return f - F(np.median(f))
    return RC.blob(sizes) if kind == "blob" else RC.closed_field(sizes)


def _random_rays(sizes, n, seed):
    """rays at the box: origins around and inside it (and so inside the surface), every eighth direction axis-parallel"""
    rng = np.random.default_rng(seed)
    D = len(sizes)
    hi = np.array(sizes, np.float64) - 1
    o = rng.uniform(-0.4, 1.4, size=(n, D)) * hi
    o[::3] = rng.uniform(0.2, 0.8, size=(len(o[::3]), D)) * hi
    target = rng.uniform(0.1, 0.9, size=(n, D)) * hi
    d = (target - o) * rng.uniform(0.05, 3.0, size=(n, 1))
    d[::8] = RC.axis_directions(D)[rng.integers(0, 2 * D, size=len(d[::8]))]
    return o.astype(F), d.astype(F)


def _check_rays(fi, f, sizes, o, d, what, **kw):
    side = kw.pop("side", ref.FRONT)
    want = ref.raycast(f, sizes, o, d, side=side, **kw)
    got = fi.raycast_field(f, sizes, o, d, side=SIDES[side], positions=True, normals=True, **kw)
    for name, g, w in zip(("t", "side", "positions", "normals"), got, (want[0], want[3], want[1], want[2])):
        _bits_equal(g, w, (what, name))
    return want


@pytest.mark.parametrize("kind,sizes", [("blob", [9, 7, 8]), ("open", [9, 7, 8]), ("blob", [12, 11, 10]), ("open", [12, 11, 10]),
                                        ("closed", [31, 17]), ("open", [31, 17]), ("closed", [24, 24, 24])], ids=str)
def test_rays_equal_the_definition(fi, kind, sizes):
    f = _field(kind, sizes)
    D = len(sizes)
    # every lattice point along the 2 D axis directions: exactly axis-parallel rays through lattice lines and faces
    p = RC.lattice_points(sizes).astype(F)
    if len(p) > 2000:
        p = p[::7]
    axes = RC.axis_directions(D)
    o, d = np.repeat(p, len(axes), axis=0), np.tile(axes, (len(p), 1))
    want = _check_rays(fi, f, sizes, o, d, "lattice lines", side=ref.EITHER)
    assert (want[3] != 0).sum() > len(o) // 10
    o, d = _random_rays(sizes, 4096, 11 + sum(sizes))
    for side in SIDES:
        want = _check_rays(fi, f, sizes, o, d, ("random", side), side=side)
        assert (want[3] != 0).sum() > 400
    for n in (0, 1, 63, 64, 65, 257):
        _check_rays(fi, f, sizes, o[:n], d[:n], ("count", n), side=ref.EITHER)


@pytest.mark.parametrize("step", [0.37, 1.0, 2.5])
@pytest.mark.parametrize("refine", [0, 1, 4, 16])
def test_steps_and_refinements(fi, step, refine):
    sizes = [12, 11, 10]
    o, d = _random_rays(sizes, 1024, 3)
    for kind in ("blob", "open"):
        want = _check_rays(fi, _field(kind, sizes), sizes, o, d, (kind, step, refine), step=step, refine=refine, side=ref.EITHER)
        assert (want[3] != 0).sum() > 100
    o2, d2 = _random_rays([31, 17], 512, 4)
    _check_rays(fi, _field("open", [31, 17]), [31, 17], o2, d2, ("2-D", step, refine), step=step, refine=refine, side=ref.EITHER, iso=0.2)


def test_iso_weights_windows_and_rays_that_are_none(fi):
    sizes = [12, 11, 10]
    f = _field("open", sizes)
    o, d = _random_rays(sizes, 2048, 5)
    for iso in (-0.3, 0.45):
        assert (_check_rays(fi, f, sizes, o, d, ("iso", iso), iso=iso, side=ref.EITHER)[3] != 0).sum() > 200
    rng = np.random.default_rng(6)
    W = rng.uniform(0.0, 2.0, size=f.size).astype(F)
    W[rng.integers(0, 9, size=f.size) == 0] = 0.0            # holes
    W[rng.integers(0, 50, size=f.size) == 0] = np.nan
    hits = [(_check_rays(fi, f, sizes, o, d, ("weight", mw), weight=W, min_weight=mw, side=ref.EITHER)[3] != 0).sum() for mw in (0.0, 0.6)]
    free = (ref.raycast(f, sizes, o, d, side=ref.EITHER)[3] != 0).sum()
    assert 0 < hits[1] < hits[0] < free
    g = f.copy()
    g[rng.integers(0, 40, size=f.size) == 0] = np.nan          # non-finite values end brackets
    g[7] = np.inf
    _check_rays(fi, g, sizes, o, d, "non-finite field", side=ref.EITHER)
    # windows: one that excludes every crossing, negative t, a window inside the box
    full = ref.raycast(f, sizes, o, d, side=ref.EITHER, t_min=-np.inf)
    first = float(np.min(full[0][np.isfinite(full[0])]))
    want = _check_rays(fi, f, sizes, o, d, "window before", side=ref.EITHER, t_min=-np.inf, t_max=first - 1.0)
    assert not want[3].any()
    _check_rays(fi, f, sizes, o, d, "window negative", side=ref.EITHER, t_min=-np.inf, t_max=0.25)
    _check_rays(fi, f, sizes, o, d, "window inside", side=ref.EITHER, t_min=0.3, t_max=0.6)
    _check_rays(fi, f, sizes, o, d, "window of one point", side=ref.EITHER, t_min=0.5, t_max=0.5)
    # rays that are none, rays beside the box, huge and tiny directions
    bo = np.array([[np.nan, 3, 3], [0, np.inf, 3], [0, 3, 3], [0, 3, 3], [0, 3, 3], [-4, 3, 3], [3, 3, -2], [1, 1, 1], [1, 1, 1], [3e38, 1, 1]], F)
    bd = np.array([[1, 0, 0], [1, 0, 0], [0, 0, 0], [np.nan, 0, 0], [1, -np.inf, 0], [0, 1, 0], [0, 0, -1], [1e30, 1e30, 0], [1e-30, 0, 0], [-1, 0, 0]], F)
    want = _check_rays(fi, f, sizes, bo, bd, "none", side=ref.EITHER)
    assert np.isnan(want[0][:5]).all() and np.isposinf(want[0][5:7]).all()


def test_outputs_left_out_memory_kinds_and_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    sizes = [9, 7, 8]
    f = _field("blob", sizes)
    o, d = _random_rays(sizes, 257, 8)
    want = ref.raycast(f, sizes, o, d, side=ref.EITHER)
    opt = _capi.FiMarchOptions()
    assert L.fi_march_default_options(C.byref(opt)) == 0
    assert (opt.iso, opt.step, opt.min_weight, opt.refine, opt.side) == (0.0, 1.0, 0.0, 4, 0)
    opt.side = ref.EITHER
    sz = (C.c_int * 3)(*sizes)
    n = len(o)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def cast(keep, options=opt, field=f, ndim=3, szs=sz, count=n, tmin=0.0, tmax=math.inf, memory=0):
        outs = [np.full(n, 7, F), np.full((n, 3), 7, F), np.full((n, 3), 7, F), np.full(n, 7, np.int8)]
        args = [a if k else None for a, k in zip(outs, keep)]
        rc = L.fi_field_raycast(ptr(field), None, ndim, szs, C.byref(options) if options else None, count, ptr(o), ptr(d), tmin, tmax,
                                *[ptr(a) for a in args], memory)
        return rc, outs
    for leave in range(4):                                                  # each output left out in turn
        keep = [k != leave for k in range(4)]
        rc, outs = cast(keep)
        assert rc == 0
        for k, (g, w) in enumerate(zip(outs, want)):
            if keep[k]:
                _bits_equal(g, w, ("left out", leave, k))
            else:
                assert (g == 7).all()
    INVALID, STATE, UNSUPPORTED = 1, 3, 5
    assert cast([False] * 4)[0] == INVALID                                   # every output NULL
    for bad in (dict(iso=math.nan), dict(iso=math.inf), dict(step=0.0), dict(step=-1.0), dict(step=math.inf), dict(step=math.nan),
                dict(refine=-1), dict(refine=17), dict(side=3), dict(side=-1), dict(min_weight=math.nan)):
        o2 = _capi.FiMarchOptions(0.0, 1.0, 0.0, 4, 0)
        for k, v in bad.items():
            setattr(o2, k, v)
        assert cast([True] * 4, options=o2)[0] == INVALID, bad
    assert cast([True] * 4, options=None)[0] == INVALID and cast([True] * 4, field=None)[0] == INVALID
    assert cast([True] * 4, count=-1)[0] == INVALID and cast([True] * 4, memory=2)[0] == INVALID
    assert cast([True] * 4, tmin=1.0, tmax=0.5)[0] == INVALID and cast([True] * 4, tmin=math.nan)[0] == INVALID
    assert cast([True] * 4, tmax=math.nan)[0] == INVALID
    assert cast([True] * 4, count=0)[0] == 0
    assert cast([True] * 4, ndim=1)[0] == UNSUPPORTED and cast([True] * 4, count=2 ** 31)[0] == UNSUPPORTED
    assert cast([True] * 4, szs=(C.c_int * 3)(9, 1, 8))[0] == INVALID and cast([True] * 4, ndim=4)[0] == INVALID
    assert L.fi_field_raycast(ptr(f), None, 3, sz, C.byref(opt), n, None, ptr(d), 0.0, 1.0, ptr(want[0].copy()), None, None, None, 0) == INVALID
    # an image: a 2-D field has no entry; a bad camera; a NULL depth
    cam = _camera(fi, cases.sphere_camera(8))._c()
    depth = np.zeros(64, F)
    assert L.fi_field_render(ptr(f), None, sz, C.byref(opt), C.byref(cam), None, None, None, None, 0) == INVALID
    assert L.fi_field_render(ptr(f), None, sz, C.byref(opt), None, ptr(depth), None, None, None, 0) == INVALID
    cam.fx = 0.0
    assert L.fi_field_render(ptr(f), None, sz, C.byref(opt), C.byref(cam), ptr(depth), None, None, None, 0) == INVALID
    cam = _camera(fi, cases.sphere_camera(8))._c()
    cam.width, cam.height = 65536, 32768
    assert L.fi_field_render(ptr(f), None, sz, C.byref(opt), C.byref(cam), ptr(depth), None, None, None, 0) == UNSUPPORTED
    cam = _camera(fi, cases.sphere_camera(8))._c()
    # contexts: before a solve, 1-D and 2-D
    lat = fi.LatticeField(sizes)
    t = np.zeros(n, F)
    assert L.fi_raycast_field(lat._h, None, C.byref(opt), n, ptr(o), ptr(d), 0.0, math.inf, ptr(t), None, None, None, 0) == STATE
    assert L.fi_render_field(lat._h, None, C.byref(opt), C.byref(cam), ptr(depth), None, None, None, 0) == STATE
    assert L.fi_raycast_field(lat._h, ptr(f), C.byref(opt), n, ptr(o), ptr(d), 0.0, math.inf, ptr(t), None, None, None, 0) == 0
    _bits_equal(t, want[0], "fi_raycast_field with a field")
    one, two = fi.LatticeField([16]), fi.LatticeField([8, 8])
    g = np.zeros(64, F)
    assert L.fi_raycast_field(one._h, ptr(g), C.byref(opt), 1, ptr(o), ptr(d), 0.0, 1.0, ptr(t), None, None, None, 0) == UNSUPPORTED
    assert L.fi_render_field(two._h, ptr(g), C.byref(opt), C.byref(cam), ptr(depth), None, None, None, 0) == UNSUPPORTED
    assert L.fi_volume_raycast(None, C.byref(opt), n, ptr(o), ptr(d), 0.0, 1.0, ptr(t), None, None, None, 0) == INVALID
    assert L.fi_volume_render(None, C.byref(opt), C.byref(cam), ptr(depth), None, None, None, 0) == INVALID
    with pytest.raises(ValueError):
        fi.raycast_field(f, sizes, o, d, side="top")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_contexts_solution(fi, dtype):
    sizes = [20, 18, 16]
    rng = np.random.default_rng(0)
    dirs = rng.normal(size=(400, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    pos = ((np.array(sizes) - 1) / 2.0 + 5.0 * dirs).astype(F)
    lat = fi.sdf_from_points(sizes, fi.Weights(), pos, dirs.astype(F), dtype=dtype)
    lat.solve_cg(None, 200, 1e-4)
    x = lat.solution_f64().astype(F)                       # an FI_F64 solution is rounded to fp32 once
    o, d = _random_rays(sizes, 1000, 9)
    want = ref.raycast(x, sizes, o, d, side=ref.EITHER, step=0.7)
    got = lat.raycast(o, d, side="either", step=0.7, positions=True, normals=True)
    for name, g, w in zip(("t", "side", "positions", "normals"), got, (want[0], want[3], want[1], want[2])):
        _bits_equal(g, w, (dtype, name))
    assert (want[3] != 0).sum() > 300
    cam = dref.look_at([40.0, 9.0, 30.0], (np.array(sizes) - 1) / 2.0, (0, 0, 1), math.radians(40.0), 33, 17, dref.Z)
    wd = ref.render(x, sizes, cam)
    gd = lat.render(_camera(fi, cam), positions=True, normals=True, incidence=True)
    _bits_equal(gd[0].reshape(-1), wd[0], (dtype, "depth"))
    for k in (1, 2, 3):
        _bits_equal(gd[k], wd[k], (dtype, "image", k))
    _bits_equal(lat.render(_camera(fi, cam), solution=x).reshape(-1), wd[0], (dtype, "a given solution"))


@pytest.mark.parametrize("hw", [(1, 1), (7, 9), (8, 8), (17, 65)], ids=str)
@pytest.mark.parametrize("kind", [dref.Z, dref.RANGE])
def test_images_equal_the_definition(fi, hw, kind):
    """widths and heights off the 8 x 8 tile: every pixel is written once, with its own ray"""
    sizes = [12, 11, 10]
    f = _field("blob", sizes)
    cam = dref.look_at([25.0, -9.0, 14.0], [5.5, 5.0, 4.5], (0, 0, 1), math.radians(20.0), hw[1], hw[0], kind)
    want = ref.render(f, sizes, cam, step=0.8)
    assert hw == (1, 1) or 0 < np.isfinite(want[0]).sum() < want[0].size
    c = _camera(fi, cam)
    got = fi.render_field(f, sizes, c, step=0.8, positions=True, normals=True, incidence=True)
    assert got[0].shape == hw
    _bits_equal(got[0].reshape(-1), want[0], "depth")
    for k in (1, 2, 3):
        _bits_equal(got[k], want[k], ("image", k))
    _bits_equal(fi.render_field(f, sizes, c, step=0.8).reshape(-1), want[0], "depth alone")
    for k, only in ((1, dict(positions=True)), (2, dict(normals=True)), (3, dict(incidence=True))):   # each optional output
        _bits_equal(fi.render_field(f, sizes, c, step=0.8, **only)[1], want[k], ("alone", k))
    back = ref.render(f, sizes, cam, step=0.8, side=ref.BACK, iso=0.3)
    got = fi.render_field(f, sizes, c, step=0.8, side="back", iso=0.3, normals=True, incidence=True)
    _bits_equal(got[0].reshape(-1), back[0], "back depth")
    assert not got[1].any() and not got[2].any()


@pytest.mark.parametrize("n", [16, 32])
def test_a_volume_renders_as_the_definition(fi, n):
    sizes = [n, n, n]
    centre = 0.5 * (n - 1.0)
    if n == 32:
        t, W = cases.fused(cases.SPHERE)
        cam = cases.sphere_camera(65)
    else:                                                  # a small volume fused on the device from three random-ish views
        rng = np.random.default_rng(2)
        cams = [dref.look_at(centre + 30.0 * np.eye(3)[a], [centre] * 3, (0, 0, 1) if a < 2 else (0, 1, 0), math.radians(40.0), 40, 40) for a in range(3)]
        depths = [(30.0 - 4.0 + rng.uniform(-0.5, 0.5, size=(40, 40))).astype(F) for _ in cams]
        t, W = dref.integrate(sizes, 2.0, 8.0, *dref.fresh(sizes), cams, depths)
        cam = dref.look_at([centre + 22.0, centre + 6.0, centre + 9.0], [centre] * 3, (0, 0, 1), math.radians(50.0), 33, 31, dref.Z)
    vol = fi.DepthVolume(sizes, 3.0 if n == 32 else 2.0, 64.0).load(t, W)
    for mw in (0.0, 1.0):
        want = ref.render(t, sizes, cam, weight=W, min_weight=mw)
        got = vol.render(_camera(fi, cam), min_weight=mw, positions=True, normals=True, incidence=True)
        _bits_equal(got[0].reshape(-1), want[0], ("volume depth", mw))
        for k in (1, 2, 3):
            _bits_equal(got[k], want[k], ("volume image", mw, k))
        assert np.isfinite(want[0]).sum() > 50
    o, d = _random_rays(sizes, 1500, 12)
    want = ref.raycast(t, sizes, o, d, weight=W, side=ref.EITHER, step=0.6)
    got = vol.raycast(o, d, side="either", step=0.6, positions=True, normals=True)
    for name, g, w in zip(("t", "side", "positions", "normals"), got, (want[0], want[3], want[1], want[2])):
        _bits_equal(g, w, ("volume rays", name))
    assert (want[3] != 0).sum() > 100


def test_a_render_feeds_the_depth_unit(fi):
    """positions of a render against depth_to_points of its depth; the image and its incidences into a fresh volume"""
    t, W = cases.fused(cases.SPHERE)
    src = fi.DepthVolume(cases.SIZES, cases.TRUNCATION, 64.0).load(t, W)
    fresh = fi.DepthVolume(cases.SIZES, cases.TRUNCATION, 64.0)
    for e in cases.eyes()[:6]:
        cam = _camera(fi, dref.look_at(e, cases.CENTRE, cases.up_for(e), cases.FOV, 96, 96, dref.RANGE))
        depth, pos, inc = src.render(cam, positions=True, incidence=True)
        back, valid = fi.depth_to_points(cam, depth, normals=False, incidence=False)
        hit = np.isfinite(depth).reshape(-1)
        assert np.array_equal(valid, hit) and hit.sum() > 1500
        # over 100 fp32 ulps at these coordinates: the two paths round differently
        assert np.abs(back[hit] - pos[hit]).max() < 1e-3
        fresh.integrate(cam, depth, inc)
    a, Wa = fresh.tsdf(), fresh.weight()
    band = (Wa > 0) & (np.abs(a) < 1) & (W > 0) & (np.abs(t) < 1)
    far = band & (np.abs(t) * cases.TRUNCATION > 0.25)                       # beyond a quarter cell the sign agrees
    assert far.sum() > 1000 and (np.sign(a[far]) == np.sign(t[far])).all()


def test_field_rays_and_mesh_rays_agree(fi):
    """hits of raycast_field and of SurfaceIndex.raycast on iso_surface of the same closed field lie in the same or in
    face-adjacent cells; at most 2 % of the rays hit exactly one of the two.  The ray set, aimed well inside the ball so that
    few rays graze it, was chosen with both restatements on the CPU (march_reference.raycast, ray_reference.raycast): 4 095 of
    the 4 096 rays hit both, none exactly one, and every pair of hits shares a cell or a face."""
    sizes = [24, 24, 24]
    f = _field("closed", sizes)
    rng = np.random.default_rng(21)
    hi = np.array(sizes, np.float64) - 1
    c = 0.5 * hi
    o = c + 1.7 * hi * (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(4096, 3)))
    target = c + rng.uniform(-0.2, 0.2, size=(4096, 3)) * hi               # aimed well inside the ball: few grazing rays
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o, d = o.astype(F), d.astype(F)
    t, sd, pos = fi.raycast_field(f, sizes, o, d, step=0.5, refine=8, positions=True)
    mesh = fi.iso_surface(f, sizes)
    tm, prim = fi.SurfaceIndex.from_mesh(mesh).raycast(o, d)
    a, b = sd != 0, prim >= 0
    print("field against mesh: %d rays, %d hit both, %d exactly one" % (len(o), (a & b).sum(), (a != b).sum()))
    assert (a != b).sum() <= 0.02 * len(o) and (a & b).sum() > 3000
    pm = o[a & b].astype(np.float64) + tm[a & b, None].astype(np.float64) * d[a & b]
    cells = np.abs(np.floor(pm) - np.floor(pos[a & b].astype(np.float64)))
    assert (cells.sum(1) <= 1).all()


def test_tracking_equals_the_restatement_chain(fi):
    true, guess, errors, cam, total, log = cases.tracked(3.0, 1.0, 2)
    _, depth, _ = cases.tracking_case(3.0, (0.5, -0.4, 0.3))
    t, W = cases.fused(cases.THREE)
    vol = fi.DepthVolume(cases.SIZES, cases.TRUNCATION, 64.0).load(t, W)
    got, info = vol.track(_camera(fi, guess), depth.reshape(48, 48), rounds=2)
    assert np.array_equal(got.pose, cam.pose)
    assert np.array_equal(info["correction"].view(np.uint64), total.view(np.uint64))
    assert info["rendered"] == [lg["rendered"] for lg in log] and info["unprojected"] == [lg["unprojected"] for lg in log]
    assert info["iterations"] == log[-1]["registration"]["iterations"] and info["counted"] == log[-1]["registration"]["counted"]
    a, s = cases.pose_errors(true, dref.Cam(got.pose, got.fx, got.fy, got.cx, got.cy, 48, 48, dref.RANGE))
    assert a <= errors[0][0] / 5 and s <= errors[0][1] / 5


def test_device_tensors(fi, tmp_path):
    """the same calls on torch tensors that live on the device, in a fresh process (tests/march_torch_worker.py), as torch
    must stay out of this one"""
    sizes = [12, 11, 10]
    f = _field("open", sizes)
    o, d = _random_rays(sizes, 700, 13)
    rng = np.random.default_rng(14)
    W = rng.uniform(0.0, 2.0, size=f.size).astype(F)
    cam = dref.look_at([25.0, -9.0, 14.0], [5.5, 5.0, 4.5], (0, 0, 1), math.radians(35.0), 21, 13, dref.RANGE)
    true, depth, guess = cases.tracking_case(3.0, (0.5, -0.4, 0.3))
    t, Wt = cases.fused(cases.THREE)
    np.savez(tmp_path / "in.npz", field=f, weight=W, sizes=np.array(sizes), o=o, d=d, pose=cam.pose, intr=np.array([cam.fx, cam.fy, cam.cx, cam.cy], F),
             shape=np.array([cam.width, cam.height, cam.kind]), tsdf=t, wt=Wt, guess=guess.pose,
             gintr=np.array([guess.fx, guess.fy, guess.cx, guess.cy], F), depth=depth)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "march_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.load(tmp_path / "out.npz")
    assert out["on_device"].all()
    want = ref.raycast(f, sizes, o, d, weight=W, min_weight=0.5, side=ref.EITHER)
    for name, w in zip(("t", "positions", "normals", "side"), want):
        _bits_equal(out["ray_" + name], w, ("device rays", name))
    want = ref.render(f, sizes, cam, weight=W, min_weight=0.5)
    for name, w in zip(("depth", "positions", "normals", "incidence"), want):
        _bits_equal(out["img_" + name].reshape(w.shape), w, ("device image", name))
    want = ref.render(t, cases.SIZES, guess, weight=Wt)
    for name, w in zip(("depth", "positions", "normals", "incidence"), want):
        _bits_equal(out["vol_" + name].reshape(w.shape), w, ("device volume image", name))
    _, _, _, cam2, total, _ = cases.tracked(3.0, 1.0, 2)
    assert np.array_equal(out["track_pose"], cam2.pose) and np.array_equal(out["track_correction"].view(np.uint64), total.view(np.uint64))
