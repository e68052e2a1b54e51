"""Depth images on the device (fi_depth.hip through fi_depth_unproject, fi_volume_* and fi_add_volume) against the numpy
definition of the contract (tests/depth_reference.py): every output as bit patterns (a NaN matches a NaN).  Lattices past
one wave in x and off any tile in y and z; images of 33 x 17, 1 x 1 and 96 x 96; both depth kinds; 1, 3 and C - 1, C, C + 1
images for the C images a launch applies; cameras outside and inside the lattice and one that misses it (the cull); depths
that are +inf, NaN, 0 and negative; incidences and image weights, a zero weight among them; a pre-loaded volume, the weight
clamp, two calls against one; the constraint list and its two-call count; fi_add_volume against fi_add_points; the error
codes; device tensors in a fresh process; and the round trip mesh -> depth images -> volume -> solve -> mesh."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_reference as ref

pytestmark = pytest.mark.gpu

F = np.float32
LATTICES = [[70, 9, 5], [20, 18, 16], [64, 4, 1]]
IMAGES = [(17, 33), (1, 1), (96, 96)]           # (height, width)
CAMS = ref.CAMERAS


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1 and _capi.FI_DEPTH_CAMERAS == CAMS
    return fi


def _bits_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.dtype == np.float32:
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    else:
        same = got == want
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:5].tolist())


def _camera(fi, c):
    return fi.Camera(c.pose, c.fx, c.fy, c.cx, c.cy, c.width, c.height, "z" if c.kind == ref.Z else "range")


def _views(sizes, m, seed):
    """m cameras around (and in, and beside) the lattice with a depth image, an incidence image and a weight each"""
    rng = np.random.default_rng(seed)
    centre = 0.5 * (np.asarray(sizes, np.float64) - 1)
    reach = float(np.linalg.norm(centre)) + 1.0
    cams, depths, incs, weights = [], [], [], []
    for s in range(m):
        h, w = IMAGES[s % 3]
        kind = ref.RANGE if s % 2 == 0 else ref.Z
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        mode = s % 4
        if mode == 1:                                  # inside the lattice: the voxels behind it are skipped
            eye, target, dist = centre + 0.3 * d, centre + 5.0 * d, 0.6 * reach
        elif mode == 3:                                # beside the lattice, looking away: the whole image misses it
            eye, target, dist = centre + 3.0 * reach * d, centre + 6.0 * reach * d, reach
        else:
            eye, target, dist = centre + 2.0 * reach * d, centre + rng.normal(size=3), 2.0 * reach
        up = np.cross(d, rng.normal(size=3))
        cams.append(ref.look_at(eye, target, up, math.radians(40.0 + 10.0 * (s % 3)), w, h, kind))
        img = (dist + rng.uniform(-0.6 * reach, 0.6 * reach, size=(h, w))).astype(F)
        bad = rng.integers(0, 12, size=(h, w))
        for code, value in ((0, np.inf), (1, np.nan), (2, 0.0), (3, -2.0)):
            img[bad == code] = value
        depths.append(img)
        q = rng.uniform(0.2, 1.0, size=(h, w)).astype(F)
        q[rng.integers(0, 25, size=(h, w)) == 0] = np.nan
        incs.append(q)
        weights.append(0.0 if s == 2 else float(rng.uniform(0.5, 2.0)))
    return cams, depths, incs, np.asarray(weights, F)


@pytest.mark.parametrize("sizes", LATTICES, ids=str)
@pytest.mark.parametrize("m", [1, 3, CAMS - 1, CAMS, CAMS + 1])
def test_integrate_equals_the_definition(fi, sizes, m):
    cams, depths, incs, weights = _views(sizes, m, 100 + m)
    for with_inc, with_w in ((False, False), (True, True), (True, False)):
        vol = fi.DepthVolume(sizes, 2.5, 4.0)
        vol.integrate([_camera(fi, c) for c in cams], depths, incs if with_inc else None, weights if with_w else None, min_incidence=0.4)
        want = ref.integrate(sizes, 2.5, 4.0, *ref.fresh(sizes), cams, depths, incs if with_inc else None, weights if with_w else None, 0.4)
        _bits_equal(vol.tsdf(), want[0], ("tsdf", with_inc, with_w))
        _bits_equal(vol.weight(), want[1], ("weight", with_inc, with_w))
        assert m < 3 or (want[1] > 0).any()


def test_a_loaded_volume_the_clamp_and_two_calls_against_one(fi):
    sizes = [70, 9, 5]
    cams, depths, incs, weights = _views(sizes, 2 * CAMS + 3, 7)
    rng = np.random.default_rng(8)
    t0 = rng.uniform(-1.0, 1.0, size=int(np.prod(sizes))).astype(F)
    W0 = rng.uniform(0.0, 3.0, size=t0.size).astype(F)
    W0[::7] = 0.0
    vol = fi.DepthVolume(sizes, 2.0, 3.0).load(t0, W0)
    _bits_equal(vol.tsdf(), t0, "loaded tsdf")
    _bits_equal(vol.weight(), W0, "loaded weight")
    fc = [_camera(fi, c) for c in cams]
    vol.integrate(fc, depths, incs, weights, min_incidence=0.3)
    want = ref.integrate(sizes, 2.0, 3.0, t0, W0, cams, depths, incs, weights, 0.3)
    _bits_equal(vol.tsdf(), want[0], "tsdf")
    _bits_equal(vol.weight(), want[1], "weight")
    assert want[1].max() == F(3.0)                                      # max_weight is reached
    two = fi.DepthVolume(sizes, 2.0, 3.0).load(t0, W0)
    cut, pix = 5, sum(d.size for d in depths[:5])
    two.integrate(fc[:cut], depths[:cut], incs[:cut], weights[:cut], min_incidence=0.3)
    two.integrate(fc[cut:], np.concatenate([d.reshape(-1) for d in depths])[pix:], incs[cut:], weights[cut:], min_incidence=0.3)
    _bits_equal(two.tsdf(), want[0], "two calls, tsdf")
    _bits_equal(two.weight(), want[1], "two calls, weight")
    again = fi.DepthVolume(sizes, 2.0, 3.0).load(t0, W0).integrate(fc, depths, incs, weights, min_incidence=0.3)
    _bits_equal(again.tsdf(), vol.tsdf(), "a repeated call")
    none = fi.DepthVolume(sizes, 2.0, 3.0).load(t0, W0).integrate([], [])
    _bits_equal(none.tsdf(), t0, "m = 0")


def test_the_cull_changes_no_result(fi, monkeypatch):
    sizes = [70, 9, 5]
    cams, depths, incs, weights = _views(sizes, CAMS + 4, 11)
    fc = [_camera(fi, c) for c in cams]
    with_cull = fi.DepthVolume(sizes, 2.5).integrate(fc, depths)
    monkeypatch.setenv("FI_NO_DEPTH_CULL", "1")
    without = fi.DepthVolume(sizes, 2.5).integrate(fc, depths)
    monkeypatch.delenv("FI_NO_DEPTH_CULL")
    _bits_equal(with_cull.tsdf(), without.tsdf(), "tsdf")
    _bits_equal(with_cull.weight(), without.weight(), "weight")
    # a camera whose whole image misses the lattice leaves the volume as it was
    away = [c for s, c in enumerate(cams) if s % 4 == 3]
    vol = fi.DepthVolume(sizes, 2.5).integrate([_camera(fi, c) for c in away], [np.full((c.height, c.width), 5.0, F) for c in away])
    assert not vol.weight().any() and (vol.tsdf() == 1).all()


@pytest.mark.parametrize("kind", ["range", "z"])
@pytest.mark.parametrize("image", IMAGES, ids=str)
def test_depth_to_points_equals_the_definition(fi, kind, image):
    h, w = image
    rng = np.random.default_rng(h + w)
    cam = ref.look_at([40.0, 3.0, 9.0], [10.0, 9.0, 8.0], (0.0, 0.0, 1.0), math.radians(50.0), w, h, ref.Z if kind == "z" else ref.RANGE)
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    depth = (30.0 + 0.05 * cols + 0.03 * rows + rng.normal(scale=0.02, size=(h, w))).astype(F)
    depth[rows > 0.7 * h] += F(4.0)                                    # a jump
    bad = rng.integers(0, 30, size=(h, w))
    for code, value in ((0, np.inf), (1, np.nan), (2, 0.0), (3, -1.0)):
        depth[bad == code] = value
    fc = _camera(fi, cam)
    for max_jump in (math.inf, 1.0, 0.0):
        want = ref.unproject(cam, depth, max_jump)
        got = fi.depth_to_points(fc, depth, max_jump)
        for g, x, name in zip(got, want, ("positions", "normals", "incidence", "valid")):
            _bits_equal(np.asarray(g).view(np.uint8) if name == "valid" else g, x, (name, max_jump))
    want = ref.unproject(cam, depth, 1.0)
    for leave in range(4):                                             # every output left out in turn
        flags = [i != leave for i in range(4)]
        got = fi.depth_to_points(fc, depth, 1.0, *flags)
        assert len(got) == 3
        for g, x in zip(got, [x for i, x in enumerate(want) if i != leave]):
            _bits_equal(np.asarray(g).view(np.uint8) if g.dtype == np.bool_ else g, x, ("without", leave))
    ok = want[3].astype(bool)
    got = fi.depth_to_points(fc, depth, 1.0, compact=True)
    for g, x in zip(got[:3], want[:3]):
        _bits_equal(g, x[ok], "compact")
    assert got[3].all() and len(got[3]) == ok.sum()
    only = fi.depth_to_points(fc, depth, 1.0, normals=False, incidence=False, valid=False, compact=True)
    assert len(only) == 1 and np.isfinite(only[0]).all() and len(only[0]) == ok.sum()


def _fused(fi, sizes, truncation=2.5, max_weight=4.0, m=5, seed=3):
    cams, depths, incs, weights = _views(sizes, m, seed)
    vol = fi.DepthVolume(sizes, truncation, max_weight).integrate([_camera(fi, c) for c in cams], depths, incs, min_incidence=0.3)
    return vol, ref.integrate(sizes, truncation, max_weight, *ref.fresh(sizes), cams, depths, incs, None, 0.3)


@pytest.mark.parametrize("sizes", LATTICES, ids=str)
def test_constraints_equal_the_definition(fi, sizes):
    from field_interpolation_amd import _capi
    vol, (t, W) = _fused(fi, sizes)
    for min_weight in (0.0, 1.5, 100.0):
        want = ref.constraints(sizes, 2.5, 4.0, t, W, min_weight)
        got = vol.constraints(min_weight)
        for g, x, name in zip(got, want, ("positions", "values", "weights")):
            _bits_equal(g, x, (name, min_weight))
        n = C.c_long(-1)
        _capi.check(_capi.lib().fi_volume_constraints(vol._h, min_weight, C.byref(n), None, None, None, 0))
        assert n.value == len(want[0])                                  # the two-call count
    assert len(ref.constraints(sizes, 2.5, 4.0, t, W)[0]) > 0 and len(vol.constraints(100.0)[0]) == 0
    assert len(fi.DepthVolume(sizes, 1.0).constraints()[0]) == 0        # a fresh volume: nothing was seen
    # values alone, and too little room
    want = ref.constraints(sizes, 2.5, 4.0, t, W)
    values = np.empty(len(want[1]), F)
    n = C.c_long(len(values))
    _capi.check(_capi.lib().fi_volume_constraints(vol._h, 0.0, C.byref(n), None, C.c_void_p(values.ctypes.data), None, 0))
    _bits_equal(values, want[1], "values alone")
    n = C.c_long(len(values) - 1)
    assert _capi.lib().fi_volume_constraints(vol._h, 0.0, C.byref(n), None, C.c_void_p(values.ctypes.data), None, 0) == 1


@pytest.mark.parametrize("kernel", ["kNearestNeighbor", "kLinearInterpolation"])
def test_add_volume_equals_add_points_of_the_constraints(fi, kernel):
    sizes = [20, 18, 16]
    vol, _ = _fused(fi, sizes)
    vk = getattr(fi.ValueKernel, kernel)
    pos, val, wgt = vol.constraints(1.0)
    assert len(pos) > 50
    a = fi.LatticeField(sizes)
    a.add_field_constraints(fi.Weights())
    a.add_volume(vol, 0.7, vk, min_weight=1.0)
    b = fi.LatticeField(sizes)
    b.add_field_constraints(fi.Weights())
    # the nearest-neighbour row reads a gradient for the step to the lattice point: zero normals, as fi_add_volume passes
    b.add_points(0.7, vk, 0.0, fi.GradientKernel.kNearestNeighbor, pos, np.zeros_like(pos) if kernel == "kNearestNeighbor" else None,
                 wgt, val)
    assert a.point_count() == b.point_count() == len(pos)
    probe = np.random.default_rng(4).normal(size=a.num_unknowns)
    assert np.array_equal(a.diag(), b.diag()) and np.array_equal(a.Atb(), b.Atb())
    assert np.array_equal(a.apply_AtA(probe), b.apply_AtA(probe))
    assert a.stats()["num_data_rows"] == len(pos)
    none = fi.LatticeField(sizes)
    none.add_volume(fi.DepthVolume(sizes, 1.0), 1.0)                    # an empty band adds nothing
    assert none.point_count() == 0


def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L, INVALID, UNSUPPORTED = _capi.lib(), 1, 5
    h = C.c_void_p()
    sz = lambda *s: (C.c_int * len(s))(*s)  # noqa: E731
    nan = math.nan
    assert L.fi_volume_create(C.byref(h), 3, sz(4, 4, 4), 0.0, 64.0) == INVALID
    assert L.fi_volume_create(C.byref(h), 3, sz(4, 4, 4), nan, 64.0) == INVALID
    assert L.fi_volume_create(C.byref(h), 3, sz(4, 4, 4), 1.0, 0.0) == INVALID
    assert L.fi_volume_create(C.byref(h), 3, sz(4, 0, 4), 1.0, 64.0) == INVALID
    assert L.fi_volume_create(C.byref(h), 3, None, 1.0, 64.0) == INVALID
    assert L.fi_volume_create(None, 3, sz(4, 4, 4), 1.0, 64.0) == INVALID
    assert L.fi_volume_create(C.byref(h), 2, sz(4, 4), 1.0, 64.0) == UNSUPPORTED
    assert L.fi_volume_create(C.byref(h), 1, sz(4), 1.0, 64.0) == UNSUPPORTED
    assert L.fi_volume_create(C.byref(h), 3, sz(2048, 2048, 512), 1.0, 64.0) == UNSUPPORTED and not h.value
    vol = fi.DepthVolume([6, 5, 4], 1.0)
    good = ref.look_at([20.0, 2.0, 2.0], [2.0, 2.0, 2.0], (0.0, 0.0, 1.0), 1.0, 3, 2)
    depth = np.full(6, 18.0, F)
    dp = C.c_void_p(depth.ctypes.data)

    def cam(**change):
        c = _camera(fi, good)._c()
        for k, v in change.items():
            if k == "pose0":
                c.pose[0] = v
            else:
                setattr(c, k, v)
        return c

    def integrate(c, m=1, d=dp, min_inc=0.5, mem=0):
        return L.fi_volume_integrate(vol._h, m, C.byref(c) if c is not None else None, d, None, None, min_inc, mem)

    assert integrate(cam()) == 0 and integrate(cam(), m=0, d=None) == 0 and integrate(None, m=0, d=None) == 0
    for bad in (cam(kind=2), cam(width=0), cam(height=-1), cam(pose0=math.inf), cam(pose0=nan), cam(fx=0.0), cam(fy=-1.0), cam(cx=nan)):
        assert integrate(bad) == INVALID
        assert L.fi_depth_unproject(C.byref(bad), dp, math.inf, dp, None, None, None, 0) == INVALID
    assert integrate(cam(), min_inc=nan) == INVALID and integrate(cam(), d=None) == INVALID and integrate(None) == INVALID
    assert integrate(cam(), m=-1) == INVALID and integrate(cam(), mem=2) == INVALID
    assert integrate(cam(width=65536, height=32768)) == UNSUPPORTED           # 2^31 pixels
    assert L.fi_volume_integrate(None, 1, C.byref(cam()), dp, None, None, 0.5, 0) == INVALID
    out = np.empty(18, F)
    op = C.c_void_p(out.ctypes.data)
    c = cam()
    assert L.fi_depth_unproject(C.byref(c), dp, math.inf, op, None, None, None, 0) == 0
    assert L.fi_depth_unproject(C.byref(c), dp, math.inf, None, None, None, None, 0) == INVALID
    assert L.fi_depth_unproject(C.byref(c), None, math.inf, op, None, None, None, 0) == INVALID
    assert L.fi_depth_unproject(None, dp, math.inf, op, None, None, None, 0) == INVALID
    assert L.fi_depth_unproject(C.byref(c), dp, -1.0, op, None, None, None, 0) == INVALID
    assert L.fi_depth_unproject(C.byref(c), dp, nan, op, None, None, None, 0) == INVALID
    assert L.fi_depth_unproject(C.byref(c), dp, math.inf, op, None, None, None, 3) == INVALID
    big = np.empty(120, F)
    bp = C.c_void_p(big.ctypes.data)
    assert L.fi_volume_load(vol._h, bp, None, 0) == INVALID and L.fi_volume_load(vol._h, bp, bp, 5) == INVALID
    assert L.fi_volume_load(None, bp, bp, 0) == INVALID and L.fi_volume_copy(vol._h, None, None, 0) == INVALID
    assert L.fi_volume_copy(vol._h, bp, None, 7) == INVALID and L.fi_volume_copy(None, bp, None, 0) == INVALID
    n = C.c_long(0)
    assert L.fi_volume_constraints(vol._h, nan, C.byref(n), None, None, None, 0) == INVALID
    assert L.fi_volume_constraints(vol._h, 0.0, None, None, None, None, 0) == INVALID
    assert L.fi_volume_constraints(None, 0.0, C.byref(n), None, None, None, 0) == INVALID
    assert L.fi_volume_constraints(vol._h, 0.0, C.byref(n), None, None, None, 9) == INVALID
    field = fi.LatticeField([6, 5, 4])
    assert L.fi_add_volume(field._h, vol._h, 1.0, 0, 0.0) == 0
    assert L.fi_add_volume(field._h, None, 1.0, 0, 0.0) == INVALID and L.fi_add_volume(None, vol._h, 1.0, 0, 0.0) == INVALID
    assert L.fi_add_volume(field._h, vol._h, 1.0, 2, 0.0) == INVALID and L.fi_add_volume(field._h, vol._h, 1.0, 0, nan) == INVALID
    assert L.fi_add_volume(fi.LatticeField([6, 5, 5])._h, vol._h, 1.0, 0, 0.0) == INVALID
    assert L.fi_add_volume(fi.LatticeField([6, 5])._h, vol._h, 1.0, 0, 0.0) == UNSUPPORTED
    assert L.fi_add_volume(fi.LatticeField([6, 5, 4], rank=0, nranks=2)._h, vol._h, 1.0, 0, 0.0) == UNSUPPORTED
    assert L.fi_volume_destroy(None) == 0
    with pytest.raises(ValueError):
        vol.integrate([_camera(fi, good)], [depth[:5]])
    with pytest.raises(ValueError):
        fi.depth_to_points(_camera(fi, good), depth[:5])
    with pytest.raises(ValueError):
        fi.Camera(good.pose, 1, 1, 0, 0, 3, 2, "fisheye")


def test_device_tensors(fi, tmp_path):
    """the same calls on torch tensors that live on the device, in a fresh process (tests/depth_torch_worker.py), as torch
    must stay out of this one"""
    sizes = [20, 18, 16]
    cams, depths, incs, weights = _views(sizes, CAMS + 1, 21)
    np.savez(tmp_path / "in.npz", pose=np.stack([c.pose for c in cams]), intr=np.array([[c.fx, c.fy, c.cx, c.cy] for c in cams], F),
             shape=np.array([[c.width, c.height, c.kind] for c in cams]), depths=np.concatenate([d.reshape(-1) for d in depths]),
             incs=np.concatenate([q.reshape(-1) for q in incs]), weights=weights)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "depth_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"].all()
    t, W = ref.integrate(sizes, 2.5, 4.0, *ref.fresh(sizes), cams, depths, incs, weights, 0.3)
    _bits_equal(o["tsdf"], t, "tsdf")
    _bits_equal(o["weight"], W, "weight")
    for i, x in enumerate(ref.constraints(sizes, 2.5, 4.0, t, W, 1.0)):
        _bits_equal(o["con_%d" % i], x, ("constraints", i))
    want = ref.unproject(cams[2], depths[2], 1.0)
    for i, x in enumerate(want):
        _bits_equal(o["pts_%d" % i].view(np.uint8) if i == 3 else o["pts_%d" % i], x, ("depth_to_points", i))
    ok = want[3].astype(bool)
    for i, x in enumerate(want[:3]):
        _bits_equal(o["cmp_%d" % i], x[ok], ("compact", i))
    assert np.array_equal(o["diag_volume"], o["diag_points"])


# ---- the round trip: mesh -> depth images -> oriented points -> volume -> solve -> mesh ------------------------------------
def test_round_trip_from_a_mesh_through_depth_images_back_to_a_mesh(fi):
    sizes, centre, radius = [32, 32, 32], np.array([15.5, 15.5, 15.5]), 10.0
    X, Y, Z = ref.voxel_coordinates(sizes)
    sdf = (np.linalg.norm(np.stack([X, Y, Z], 1).astype(np.float64) - centre, axis=1) - radius).astype(F)
    source = fi.iso_surface(sdf, sizes)
    surface = fi.SurfaceIndex.from_mesh(source)
    dirs = [np.eye(3)[a] * s for a in range(3) for s in (1, -1)]
    dirs += [np.array([sx, sy, sz]) / math.sqrt(3.0) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    cams, depths, incs = [], [], []
    for d in dirs:
        eye = centre + 40.0 * d
        up = (0.0, 0.0, 1.0) if abs(d[2]) < 0.9 else (0.0, 1.0, 0.0)
        cams.append(fi.camera_look_at(eye, centre, up, math.radians(50.0), 96, 96))
        depths.append(surface.render_depth(eye, centre, up, math.radians(50.0), 96, 96)[0])
        pos, inc = fi.depth_to_points(cams[-1], depths[-1], normals=False, valid=False, compact=False)
        incs.append(inc)
        seen = np.isfinite(pos).all(1)
        assert seen.sum() > 1000
        # 1e-3 lattice units: about 100 float32 ulps of a coordinate below 128, all that t and the transform can lose
        assert surface.distance(pos[seen]).max() <= 1e-3
    # the default Weights(), and max_weight = 4: a voxel of the band is seen at an incidence >= 0.5 by at most four of the 14
    # views (W <= 3.03), and the point weights are W / max_weight -- with the default 64 they stay below 0.05, their squares
    # lose against model_2 = 0.5 and the converged surface lies two cells off
    field, volume = fi.sdf_from_depth(sizes, fi.Weights(), cams, depths, 3.0, incidences=incs, min_incidence=0.5, max_weight=4.0)
    x, iterations, residual = field.solve_cg(None, 0, 1e-6)
    mesh, parts = field.iso_surface(parts=True)
    dev = fi.mesh_deviation(mesh, source, samples=20000, seed=1)
    rms = max(dev["a_to_b"]["samples"]["rms"], dev["b_to_a"]["samples"]["rms"])
    print("round trip: %d band voxels, %d iterations, %d part(s), boundary edges %d, symmetric rms %.4f, hausdorff %.4f"
          % (field.point_count(), iterations, len(parts.vertices), int(parts.boundary.sum()), rms, dev["hausdorff"]))
    assert len(parts.vertices) == 1 and parts.boundary.sum() == 0       # one closed part
    assert rms <= 0.5                                                  # half a cell: no wrong sign, no shifted surface
