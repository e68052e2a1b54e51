"""Colour in a depth volume on the device (fi_colour.hip through fi_volume_set_channels, fi_volume_integrate_colour,
fi_volume_colour_sample, fi_volume_render_colour, fi_volume_colour_constraints) against the numpy definition of the contract
(tests/colour_reference.py): every output as bit patterns (a NaN matches a NaN).  Lattices past one wave in x, of exactly one
wave and flat; 1, C and C + 1 images for the C images a launch applies; 1, 2, 3 and 4 channels; images of 17 x 33, 1 x 1 and
24 x 24; cameras outside, inside and beside the lattice; invalid depths, NaN incidences, a zero image weight and non-finite
colour channels; tsdf and weight against DepthVolume.integrate without colours; one call against two; a loaded colour state;
the cull; samples inside, on the faces, outside and NaN; colour images; the constraint list and its two-call count; the error
codes; and device tensors in a fresh process."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import colour_reference as ref
import depth_reference as dref

pytestmark = pytest.mark.gpu

F = np.float32
LATTICES = [[70, 9, 5], [20, 18, 16], [64, 4, 1]]
IMAGES = [(17, 33), (1, 1), (24, 24)]           # (height, width)
CAMS = dref.CAMERAS


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
    return fi.Camera(c.pose, c.fx, c.fy, c.cx, c.cy, c.width, c.height, "z" if c.kind == dref.Z else "range")


def _views(sizes, m, seed, channels):
    """m cameras around (and in, and beside) the lattice with a depth image, an incidence image, a weight and a colour image
    each (the views of tests/test_gpu_depth.py, and colours with non-finite channels among them)"""
    rng = np.random.default_rng(seed)
    centre = 0.5 * (np.asarray(sizes, np.float64) - 1)
    reach = float(np.linalg.norm(centre)) + 1.0
    cams, depths, incs, weights, colours = [], [], [], [], []
    for s in range(m):
        h, w = IMAGES[s % 3]
        kind = dref.RANGE if s % 2 == 0 else dref.Z
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
        cams.append(dref.look_at(eye, target, up, math.radians(40.0 + 10.0 * (s % 3)), w, h, kind))
        img = (dist + rng.uniform(-0.6 * reach, 0.6 * reach, size=(h, w))).astype(F)
        bad = rng.integers(0, 12, size=(h, w))
        for code, value in ((0, np.inf), (1, np.nan), (2, 0.0), (3, -2.0)):
            img[bad == code] = value
        depths.append(img)
        q = rng.uniform(0.2, 1.0, size=(h, w)).astype(F)
        q[rng.integers(0, 25, size=(h, w)) == 0] = np.nan
        incs.append(q)
        weights.append(0.0 if s == 2 else float(rng.uniform(0.5, 2.0)))
        c = rng.uniform(0.0, 255.0, size=(h, w, channels)).astype(F)
        bad = rng.integers(0, 10 * channels, size=(h, w, channels))
        for code, value in ((0, np.nan), (1, np.inf), (2, -np.inf)):
            c[bad == code] = value
        colours.append(c)
    return cams, depths, incs, np.asarray(weights, F), colours


def _state(vol):
    return vol.tsdf(), vol.weight(), vol.colours(), vol.colour_weight()


def _equal_state(got, want, what):
    for g, x, name in zip(got, want, ("tsdf", "weight", "colours", "colour weight")):
        _bits_equal(g, x, (name,) + tuple(what))


def _check_integration(fi, sizes, m, channels, seed):
    cams, depths, incs, weights, colours = _views(sizes, m, seed, channels)
    fc = [_camera(fi, c) for c in cams]
    for with_inc, with_w, band in ((False, False, 1.0), (True, True, 0.6)):
        q, iw = (incs if with_inc else None), (weights if with_w else None)
        vol = fi.DepthVolume(sizes, 2.5, 4.0, channels=channels)
        vol.integrate(fc, depths, q, iw, min_incidence=0.4, colours=colours, colour_band=band)
        want = ref.integrate_colour(sizes, 2.5, 4.0, *dref.fresh(sizes), *ref.fresh(sizes, channels), cams, depths, colours, q, iw, 0.4, band)
        _equal_state(_state(vol), want, (with_inc, with_w))
        plain = fi.DepthVolume(sizes, 2.5, 4.0).integrate(fc, depths, q, iw, min_incidence=0.4)
        _bits_equal(vol.tsdf(), plain.tsdf(), "tsdf without colours")
        _bits_equal(vol.weight(), plain.weight(), "weight without colours")
        # some voxels coloured, some seen and not coloured (the narrow band may leave the flat lattice without a colour)
        assert m < 3 or band < 1.0 or ((want[3] > 0).any() and (want[3][want[1] > 0] == 0).any())


@pytest.mark.parametrize("sizes", LATTICES, ids=str)
@pytest.mark.parametrize("m", [1, CAMS, CAMS + 1])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_integrate_equals_the_definition(fi, sizes, m, channels):
    _check_integration(fi, sizes, m, channels, 100 + m)


def test_integrate_two_channels(fi):
    _check_integration(fi, [70, 9, 5], CAMS + 1, 2, 31)


def test_colours_of_any_dtype_as_one_flat_array(fi):
    sizes = [20, 18, 16]
    cams, depths, incs, weights, _ = _views(sizes, 3, 5, 3)
    rng = np.random.default_rng(6)
    bytes_ = [rng.integers(0, 256, size=(c.height, c.width, 3), dtype=np.uint8) for c in cams]
    fc = [_camera(fi, c) for c in cams]
    a = fi.DepthVolume(sizes, 2.5, 4.0, channels=3).integrate(fc, depths, colours=bytes_)
    b = fi.DepthVolume(sizes, 2.5, 4.0, channels=3).integrate(fc, depths, colours=np.concatenate([x.reshape(-1) for x in bytes_]))
    want = ref.integrate_colour(sizes, 2.5, 4.0, *dref.fresh(sizes), *ref.fresh(sizes, 3), cams, depths, [x.astype(F) for x in bytes_])
    _equal_state(_state(a), want, ("uint8 images",))
    _equal_state(_state(b), want, ("one flat uint8 array",))
    assert want[2].max() > 1.0                                          # not scaled


def test_a_loaded_state_the_clamp_and_two_calls_against_one(fi):
    sizes, channels = [70, 9, 5], 3
    cams, depths, incs, weights, colours = _views(sizes, 2 * CAMS + 3, 7, channels)
    rng = np.random.default_rng(8)
    n = int(np.prod(sizes))
    t0 = rng.uniform(-1.0, 1.0, size=n).astype(F)
    W0 = rng.uniform(0.0, 3.0, size=n).astype(F)
    W0[::7] = 0.0
    A0 = rng.uniform(0.0, 255.0, size=(channels, n)).astype(F)
    Wc0 = rng.uniform(0.0, 3.0, size=n).astype(F)
    Wc0[::5] = 0.0

    def loaded():
        return fi.DepthVolume(sizes, 2.0, 3.0, channels=channels).load(t0, W0).load_colours(A0, Wc0)

    vol = loaded()
    _equal_state(_state(vol), (t0, W0, A0, Wc0), ("loaded",))
    fc = [_camera(fi, c) for c in cams]
    vol.integrate(fc, depths, incs, weights, min_incidence=0.3, colours=colours)
    want = ref.integrate_colour(sizes, 2.0, 3.0, t0, W0, A0, Wc0, cams, depths, colours, incs, weights, 0.3)
    _equal_state(_state(vol), want, ("resumed",))
    assert want[3].max() == F(3.0)                                      # max_weight is reached
    two = loaded()
    cut = 5
    pix = sum(d.size for d in depths[:cut])
    two.integrate(fc[:cut], depths[:cut], incs[:cut], weights[:cut], min_incidence=0.3, colours=colours[:cut])
    two.integrate(fc[cut:], depths[cut:], incs[cut:], weights[cut:], min_incidence=0.3,
                  colours=np.concatenate([c.reshape(-1) for c in colours])[channels * pix:])
    _equal_state(_state(two), want, ("two calls",))
    none = loaded().integrate([], [], colours=[])
    _equal_state(_state(none), (t0, W0, A0, Wc0), ("m = 0",))
    # the geometry calls leave the colour state alone
    geo = loaded().integrate(fc, depths, incs, weights, min_incidence=0.3)
    _bits_equal(geo.colours(), A0, "colours after integrate without colours")
    _bits_equal(geo.colour_weight(), Wc0, "colour weight after integrate without colours")
    _bits_equal(geo.tsdf(), want[0], "tsdf of integrate without colours")


def test_the_cull_changes_no_result(fi, monkeypatch):
    sizes = [70, 9, 5]
    cams, depths, incs, weights, colours = _views(sizes, CAMS + 4, 11, 4)
    fc = [_camera(fi, c) for c in cams]
    with_cull = fi.DepthVolume(sizes, 2.5, channels=4).integrate(fc, depths, colours=colours)
    monkeypatch.setenv("FI_NO_DEPTH_CULL", "1")
    without = fi.DepthVolume(sizes, 2.5, channels=4).integrate(fc, depths, colours=colours)
    monkeypatch.delenv("FI_NO_DEPTH_CULL")
    _equal_state(_state(with_cull), _state(without), ("cull",))
    assert (with_cull.colour_weight() > 0).any()


# ---- a colour state to sample and render -----------------------------------------------------------------------------------
def _ball(sizes, channels, seed):
    """a ball's tsdf (truncation 2) with weights, and colours on a shell around its surface with gaps in it"""
    rng = np.random.default_rng(seed)
    X, Y, Z = dref.voxel_coordinates(sizes)
    centre = 0.5 * (np.asarray(sizes, np.float64) - 1)
    radius = 0.35 * (min(sizes) - 1) if min(sizes) > 4 else 0.4
    dist = np.linalg.norm(np.stack([X, Y, Z], 1).astype(np.float64) - centre, axis=1) - radius
    t = np.clip(dist / 2.0, -1.0, 1.0).astype(F)
    W = np.where(np.abs(dist) < 3.0, rng.uniform(0.5, 3.0, size=t.size), 0.0).astype(F)
    A = rng.uniform(0.0, 1.0, size=(channels, t.size)).astype(F)
    Wc = np.where(np.abs(dist) < 1.5, rng.uniform(0.2, 3.0, size=t.size), 0.0).astype(F)
    Wc[rng.integers(0, 4, size=t.size) == 0] = 0.0
    return t, W, A, Wc


def _queries(sizes, seed):
    rng = np.random.default_rng(seed)
    hi = np.asarray(sizes, np.float64) - 1
    inside = rng.uniform(0.0, 1.0, size=(3000, 3)) * hi
    faces = rng.uniform(0.0, 1.0, size=(600, 3)) * hi
    for i in range(len(faces)):                                         # one coordinate (or all three) exactly on a face
        j = i % 4
        if j < 3:
            faces[i, j] = (0.0, hi[j])[(i // 4) % 2]
        else:
            faces[i] = np.where(rng.integers(0, 2, size=3) == 0, 0.0, hi)
    outside = rng.uniform(-1.0, 1.0, size=(200, 3)) * 0.5 + np.where(rng.integers(0, 2, size=(200, 3)) == 0, -0.6, hi + 0.6)
    odd = np.array([[np.nan, 1.0, 0.5], [1.0, np.inf, 0.5], [1.0, 1.0, -np.inf], [-1e-6, 1.0, 0.5], [0.0, 0.0, 0.0], list(hi)])
    grid = np.floor(inside[:300])                                       # on lattice points
    return np.concatenate([inside, faces, outside, odd, grid]).astype(F)


@pytest.mark.parametrize("sizes,channels", [([20, 18, 16], 3), ([65, 3, 2], 4), ([20, 18, 16], 1), ([65, 3, 2], 2)], ids=str)
def test_samples_equal_the_definition(fi, sizes, channels):
    t, W, A, Wc = _ball(sizes, channels, 3)
    if sizes[2] == 2:                                                   # (the ball is a few voxels there: colour two thirds of all)
        rng = np.random.default_rng(4)
        Wc = np.where(rng.integers(0, 3, size=Wc.size) > 0, rng.uniform(0.3, 3.0, size=Wc.size), 0.0).astype(F)
    vol = fi.DepthVolume(sizes, 2.0, 4.0, channels=channels).load(t, W).load_colours(A, Wc)
    pts = _queries(sizes, 9)
    for min_weight in (0.0, 1.2):                                       # the second excludes some corners
        want, ok = ref.sample(sizes, A, Wc, pts, min_weight)
        got, valid = vol.sample_colours(pts, min_weight, valid=True)
        _bits_equal(got, want, ("colours", min_weight))
        _bits_equal(valid.view(np.uint8), ok, ("valid", min_weight))
        _bits_equal(vol.sample_colours(pts, min_weight), want, ("colours alone", min_weight))
        assert 0 < ok.sum() < len(ok)
    less = ref.sample(sizes, A, Wc, pts, 1.2)[1].sum()
    assert less < ref.sample(sizes, A, Wc, pts)[1].sum()
    assert vol.sample_colours(np.zeros((0, 3), F)).shape == (0, channels)


@pytest.mark.parametrize("hw", [(24, 24), (1, 1)], ids=str)
def test_colour_images_equal_the_definition(fi, hw):
    sizes, channels = [20, 18, 16], 3
    t, W, A, Wc = _ball(sizes, channels, 12)
    vol = fi.DepthVolume(sizes, 2.0, 4.0, channels=channels).load(t, W).load_colours(A, Wc)
    centre = 0.5 * (np.asarray(sizes, np.float64) - 1)
    cam = dref.look_at(centre + [22.0, 6.0, 9.0], centre, (0, 0, 1), math.radians(40.0), hw[1], hw[0], dref.Z)
    fc = _camera(fi, cam)
    for cmw in (0.0, 1.0):
        want = ref.render_colour(sizes, t, W, A, Wc, cam, step=0.8, min_weight=0.5, colour_min_weight=cmw)
        got = vol.render(fc, step=0.8, min_weight=0.5, positions=True, normals=True, incidence=True, colours=True, colour_min_weight=cmw)
        plain = vol.render(fc, step=0.8, min_weight=0.5, positions=True, normals=True, incidence=True)
        assert len(got) == 5 and len(plain) == 4
        for k, name in enumerate(("depth", "positions", "normals", "incidence")):
            _bits_equal(got[k], plain[k], ("render without colours", name))
            _bits_equal(got[k].reshape(want[k].shape), want[k], (name, cmw))
        _bits_equal(got[4], want[4], ("colours", cmw))
        _bits_equal(got[4], vol.sample_colours(got[1], cmw), ("sample_colours of the positions", cmw))
        hit = np.isfinite(want[0])
        assert hit.any() and np.isnan(want[4][~hit]).all() and np.isfinite(want[4][hit]).any()
    only = vol.render(fc, step=0.8, min_weight=0.5, colours=True)          # the depth and the colours alone
    assert len(only) == 2
    _bits_equal(only[0], plain[0], "depth alone")
    _bits_equal(only[1], ref.render_colour(sizes, t, W, A, Wc, cam, step=0.8, min_weight=0.5)[4], "colours alone")


@pytest.mark.parametrize("sizes,channels", [([70, 9, 5], 3), ([64, 4, 1], 4), ([20, 18, 16], 1)], ids=str)
def test_colour_constraints_equal_the_definition(fi, sizes, channels):
    from field_interpolation_amd import _capi
    t, W, A, Wc = _ball(sizes, channels, 5)
    vol = fi.DepthVolume(sizes, 2.0, 4.0, channels=channels).load(t, W).load_colours(A, Wc)
    for min_weight in (0.0, 1.5, 100.0):
        want = ref.constraints(sizes, 4.0, A, Wc, min_weight)
        got = vol.colour_constraints(min_weight)
        for g, x, name in zip(got, want, ("positions", "colours", "weights")):
            _bits_equal(g, x, (name, min_weight))
        n = C.c_long(-1)
        _capi.check(_capi.lib().fi_volume_colour_constraints(vol._h, min_weight, C.byref(n), None, None, None, 0))
        assert n.value == len(want[0])                                  # the two-call count
    want = ref.constraints(sizes, 4.0, A, Wc)
    assert len(want[0]) > 0 and len(vol.colour_constraints(100.0)[0]) == 0
    assert len(fi.DepthVolume(sizes, 1.0, channels=channels).colour_constraints()[0]) == 0
    colours = np.empty((len(want[0]), channels), F)                     # the colours alone, and too little room
    n = C.c_long(len(colours))
    _capi.check(_capi.lib().fi_volume_colour_constraints(vol._h, 0.0, C.byref(n), None, C.c_void_p(colours.ctypes.data), None, 0))
    _bits_equal(colours, want[1], "colours alone")
    n = C.c_long(len(colours) - 1)
    assert _capi.lib().fi_volume_colour_constraints(vol._h, 0.0, C.byref(n), None, C.c_void_p(colours.ctypes.data), None, 0) == 1


def test_a_channel_completes_by_a_solve(fi):
    """the chain of the docstrings: the coloured voxels of one channel as data points of a field"""
    sizes = [20, 18, 16]
    t, W, A, Wc = _ball(sizes, 3, 5)
    vol = fi.DepthVolume(sizes, 2.0, 4.0, channels=3).load(t, W).load_colours(A, Wc)
    pos, col, wgt = vol.colour_constraints()
    field = fi.LatticeField(sizes)
    field.add_field_constraints(fi.Weights())
    field.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kNearestNeighbor, pos, values=col[:, 1],
                     point_weights=wgt)
    assert field.point_count() == len(pos) > 100
    x, _, _ = field.solve_cg(None, 200, 1e-4)
    seen = (pos[:, 2].astype(int) * sizes[1] + pos[:, 1].astype(int)) * sizes[0] + pos[:, 0].astype(int)
    # the planted colours are noise, uniform in [0, 1]: a smooth least-squares fit stays about that range, around their mean
    assert np.isfinite(x).all() and x[seen].min() > -0.5 and x[seen].max() < 1.5 and abs(x[seen].mean() - 0.5) < 0.2


def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L, INVALID, STATE, UNSUPPORTED = _capi.lib(), 1, 3, 5
    nan = math.nan
    vol = fi.DepthVolume([6, 5, 4], 1.0)
    good = dref.look_at([20.0, 2.0, 2.0], [2.0, 2.0, 2.0], (0.0, 0.0, 1.0), 1.0, 3, 2)
    cam = _camera(fi, good)._c()
    depth, colour = np.full(6, 18.0, F), np.full(18, 0.5, F)
    big = np.empty(3 * 120, F)
    dp, cp, bp = (C.c_void_p(a.ctypes.data) for a in (depth, colour, big))
    opt = _capi.FiMarchOptions(0.0, 1.0, 0.0, 4, 0)
    n = C.c_long(0)
    k = C.c_int(-1)
    assert L.fi_volume_channels(vol._h, C.byref(k)) == 0 and k.value == 0
    assert L.fi_volume_channels(None, C.byref(k)) == INVALID and L.fi_volume_channels(vol._h, None) == INVALID

    def calls(v):
        return (L.fi_volume_colour_load(v, bp, bp, 0), L.fi_volume_colour_copy(v, bp, None, 0),
                L.fi_volume_integrate_colour(v, 1, C.byref(cam), dp, None, None, 0.5, cp, 1.0, 0),
                L.fi_volume_colour_sample(v, 0.0, 2, bp, bp, None, 0),
                L.fi_volume_render_colour(v, C.byref(opt), C.byref(cam), 0.0, bp, None, None, None, bp, 0),
                L.fi_volume_colour_constraints(v, 0.0, C.byref(n), None, None, None, 0))

    assert calls(vol._h) == (STATE,) * 6                                # no channels yet
    assert calls(None) == (INVALID,) * 6
    assert L.fi_volume_set_channels(vol._h, 0) == INVALID and L.fi_volume_set_channels(vol._h, 5) == INVALID
    assert L.fi_volume_set_channels(None, 3) == INVALID
    assert L.fi_volume_set_channels(vol._h, 3) == 0 and L.fi_volume_set_channels(vol._h, 3) == STATE
    assert L.fi_volume_channels(vol._h, C.byref(k)) == 0 and k.value == 3
    big[:] = 0.25
    assert calls(vol._h) == (0,) * 6

    def integrate(m=1, c=cp, band=1.0, d=dp, mem=0, min_inc=0.5):
        return L.fi_volume_integrate_colour(vol._h, m, C.byref(cam), d, None, None, min_inc, c, band, mem)

    assert integrate() == 0 and integrate(m=0, c=None, d=None) == 0
    assert integrate(c=None) == INVALID and integrate(d=None) == INVALID and integrate(m=-1) == INVALID and integrate(mem=2) == INVALID
    for band in (0.0, -0.5, 1.5, nan, math.inf):
        assert integrate(band=band) == INVALID
    assert integrate(band=1e-3) == 0 and integrate(min_inc=nan) == INVALID
    bad = _camera(fi, good)._c()
    bad.width = 0
    assert L.fi_volume_integrate_colour(vol._h, 1, C.byref(bad), dp, None, None, 0.5, cp, 1.0, 0) == INVALID
    assert L.fi_volume_colour_load(vol._h, bp, None, 0) == INVALID and L.fi_volume_colour_load(vol._h, bp, bp, 4) == INVALID
    assert L.fi_volume_colour_copy(vol._h, None, None, 0) == INVALID and L.fi_volume_colour_copy(vol._h, bp, None, 7) == INVALID
    assert L.fi_volume_colour_copy(vol._h, None, bp, 0) == 0
    assert L.fi_volume_colour_sample(vol._h, 0.0, 0, None, None, None, 0) == 0
    assert L.fi_volume_colour_sample(vol._h, 0.0, 2, bp, None, None, 0) == INVALID
    assert L.fi_volume_colour_sample(vol._h, 0.0, 2, None, bp, None, 0) == INVALID
    assert L.fi_volume_colour_sample(vol._h, nan, 2, bp, bp, None, 0) == INVALID
    assert L.fi_volume_colour_sample(vol._h, 0.0, -1, bp, bp, None, 0) == INVALID
    assert L.fi_volume_colour_sample(vol._h, 0.0, 2, bp, bp, None, 3) == INVALID

    def render(o=opt, c=cam, cmw=0.0, d=bp, col=bp, mem=0, v=vol._h):
        return L.fi_volume_render_colour(v, C.byref(o) if o is not None else None, C.byref(c) if c is not None else None, cmw, d, None, None,
                                         None, col, mem)

    assert render() == 0 and render(col=None) == INVALID and render(d=None) == INVALID and render(cmw=nan) == INVALID
    assert render(o=None) == INVALID and render(c=None) == INVALID and render(c=bad) == INVALID and render(mem=5) == INVALID
    assert render(o=_capi.FiMarchOptions(0.0, 0.0, 0.0, 4, 0)) == INVALID
    assert L.fi_volume_colour_constraints(vol._h, nan, C.byref(n), None, None, None, 0) == INVALID
    assert L.fi_volume_colour_constraints(vol._h, 0.0, None, None, None, None, 0) == INVALID
    assert L.fi_volume_colour_constraints(vol._h, 0.0, C.byref(n), None, None, None, 9) == INVALID
    flat = fi.DepthVolume([64, 4, 1], 1.0, channels=2)                   # a size below 2: fused and listed, not sampled
    assert L.fi_volume_colour_sample(flat._h, 0.0, 2, bp, bp, None, 0) == UNSUPPORTED
    assert render(v=flat._h) == UNSUPPORTED
    assert L.fi_volume_colour_constraints(flat._h, 0.0, C.byref(n), None, None, None, 0) == 0 and n.value == 0
    with pytest.raises(ValueError):
        fi.DepthVolume([6, 5, 4], 1.0, channels=3).integrate([_camera(fi, good)], [depth], colours=[colour[:17]])
    with pytest.raises(ValueError):
        fi.DepthVolume([6, 5, 4], 1.0, channels=3).load_colours(big[:359], big[:120])
    with pytest.raises(ValueError):
        fi.DepthVolume([6, 5, 4], 1.0, channels=3).sample_colours(np.zeros(4, F))
    with pytest.raises(Exception):
        fi.DepthVolume([6, 5, 4], 1.0, channels=5)


def test_device_tensors(fi, tmp_path):
    """the same calls on torch tensors that live on the device, in a fresh process (tests/colour_torch_worker.py), as torch
    must stay out of this one"""
    sizes, channels = [20, 18, 16], 4
    cams, depths, incs, weights, colours = _views(sizes, CAMS + 1, 21, channels)
    pts = _queries(sizes, 2)
    cam = dref.look_at([31.5, 14.5, 16.5], [9.5, 8.5, 7.5], (0, 0, 1), math.radians(40.0), 24, 24, dref.Z)
    np.savez(tmp_path / "in.npz", pose=np.stack([c.pose for c in cams + [cam]]),
             intr=np.array([[c.fx, c.fy, c.cx, c.cy] for c in cams + [cam]], F),
             shape=np.array([[c.width, c.height, c.kind] for c in cams + [cam]]), depths=np.concatenate([d.reshape(-1) for d in depths]),
             incs=np.concatenate([q.reshape(-1) for q in incs]), weights=weights, colours=np.concatenate([c.reshape(-1) for c in colours]),
             points=pts)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "colour_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"].all()
    want = ref.integrate_colour(sizes, 2.5, 4.0, *dref.fresh(sizes), *ref.fresh(sizes, channels), cams, depths, colours, incs, weights, 0.3)
    for name, x in zip(("tsdf", "weight", "colours", "colour_weight"), want):
        _bits_equal(o[name], x, name)
        _bits_equal(o["shifted_" + name], x, ("colours at an address that is no multiple of 16", name))
    t, W, A, Wc = want
    col, ok = ref.sample(sizes, A, Wc, pts, 0.5)
    _bits_equal(o["sample"], col, "sample")
    _bits_equal(o["valid"].view(np.uint8), ok, "valid")
    for i, x in enumerate(ref.constraints(sizes, 4.0, A, Wc, 1.0)):
        _bits_equal(o["con_%d" % i], x, ("constraints", i))
    img = ref.render_colour(sizes, t, W, A, Wc, cam)
    _bits_equal(o["img_depth"].reshape(-1), img[0], "image depth")
    _bits_equal(o["img_positions"], img[1], "image positions")
    _bits_equal(o["img_colours"], img[4], "image colours")
