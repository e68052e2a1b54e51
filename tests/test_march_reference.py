"""tests/march_reference.py, the numpy definition of the march unit's contract (include/fi_hip.h fi_field_raycast,
fi_field_render), held to answers known by hand: planes, windows, a weight mask, an analytic sphere, a
sphere fused from 14 views, and frame-to-model tracking on the restatement chain.  No GPU: the device is held to the same
functions bit for bit in tests/test_gpu_march.py.  The quality figures asserted here are the restatement's own, measured on the
CPU with a margin of 1.5, and are printed (pytest -s) for DESIGN.md 4.28."""
import math

import numpy as np
import pytest

import depth_reference as dref
import march_cases as cases
import march_reference as ref
import sample_reference

F = np.float32
SIZES = [9, 7, 8]
MARGIN = 1.5


def plane_field(offset=3.25):
    X, _, _ = dref.voxel_coordinates(SIZES)
    return (X - F(offset)).astype(F)


def face_rays(x, direction):
    """rays along (direction, 0, 0) from every lattice point of the face at `x`"""
    k, j = np.meshgrid(np.arange(SIZES[2]), np.arange(SIZES[1]), indexing="ij")
    o = np.stack([np.full(j.size, x), j.reshape(-1), k.reshape(-1)], 1).astype(F)
    return o, np.tile(np.array([direction, 0.0, 0.0], F), (len(o), 1))


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_planes_front_and_back(scale):
    f = plane_field()
    up, down = face_rays(0.0, scale), face_rays(8.0, -scale)          # f rises along +x: +x rays leave the inside
    for (o, d), want_t, want_side in ((up, 3.25, -1), (down, 4.75, +1)):
        worst = 0
        for refine in (0, 4):
            t, pos, nrm, sd = ref.raycast(f, SIZES, o, d, refine=refine, side=ref.EITHER)
            assert (sd == want_side).all()
            worst = max(worst, int(ulps(t, np.full(len(t), want_t / scale, F)).max()))
            assert np.abs(pos[:, 0] - F(3.25)).max() <= 2.0 ** -21 and np.array_equal(pos[:, 1:], o[:, 1:])
            assert np.array_equal(nrm, np.tile(np.array([1, 0, 0], F), (len(o), 1)))     # towards increasing f, either way
            one = ref.raycast(f, SIZES, o, d, refine=refine, side=ref.BACK if want_side < 0 else ref.FRONT)
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(one, (t, pos, nrm, sd)))
            other = ref.raycast(f, SIZES, o, d, refine=refine, side=ref.FRONT if want_side < 0 else ref.BACK)
            assert np.isposinf(other[0]).all() and np.isnan(other[1]).all() and not other[2].any() and not other[3].any()
        print("plane, d = %g, side %+d: t within %d ulp of %g at refine 0 and 4" % (scale, want_side, worst, want_t / scale))
        assert worst == 0              # the last bit, at refine 0 and at refine 4 (3.25 and 4.75 are exact in every step taken)


def test_faces_windows_misses_and_rays_that_are_none():
    f = plane_field()
    d = np.array([[1, 0, 0]], F)
    cast = lambda o, **kw: ref.raycast(f, SIZES, np.array([o], F), d, side=ref.EITHER, **kw)   # noqa: E731
    # a ray inside a face of the box is inside its slab: 0 <= o_j <= size_j - 1
    for o in ([0, 0, 0], [0, 6, 7], [0, 0, 3.5], [0, 6, 0]):
        assert cast(o)[0][0] == F(3.25)
    for o in ([0, -0.001, 3], [0, 6.001, 3], [0, 3, 7.5], [0, 3, -1]):           # parallel and outside: a miss
        t, pos, nrm, sd = cast(o)
        assert np.isposinf(t[0]) and np.isnan(pos).all() and not nrm.any() and sd[0] == 0
    # the window: both ends count
    assert cast([0, 3, 3], t_max=3.25)[0][0] == F(3.25) and np.isposinf(cast([0, 3, 3], t_max=3.2)[0][0])
    assert cast([0, 3, 3], t_min=3.0)[0][0] == F(3.25)
    assert np.isposinf(cast([0, 3, 3], t_min=3.25)[0][0]) and np.isposinf(cast([0, 3, 3], t_min=3.5)[0][0])   # beyond the crossing
    assert np.isposinf(cast([0, 3, 3], t_min=20.0, t_max=30.0)[0][0])                       # the window misses the box
    assert cast([-5, 3, 3])[0][0] == F(8.25) and cast([-5, 3, 3], t_min=-np.inf)[0][0] == F(8.25)   # from outside the box
    assert np.isposinf(ref.raycast(f, SIZES, [[9, 3, 3]], d)[0][0])                         # leaving, beside the box
    # rays that are none
    bad_o = np.array([[np.nan, 3, 3], [0, np.inf, 3], [0, 3, 3], [0, 3, 3], [0, 3, 3]], F)
    bad_d = np.array([[1, 0, 0], [1, 0, 0], [0, 0, 0], [np.nan, 0, 0], [1, -np.inf, 0]], F)
    t, pos, nrm, sd = ref.raycast(f, SIZES, bad_o, bad_d, side=ref.EITHER)
    assert np.isnan(t).all() and np.isnan(pos).all() and not nrm.any() and not sd.any()
    # a zero component of d makes no 0 * inf, and a slanted ray meets the plane where it should
    t, pos, _, sd = ref.raycast(f, SIZES, [[0.5, 0.5, 0.5]], [[1, 1, 0.5]], side=ref.EITHER, refine=8)
    assert sd[0] == -1 and abs(t[0] - 2.75) < 1e-5 and np.abs(pos[0] - np.array([3.25, 3.25, 1.875])).max() < 1e-5


def test_values_and_normals_are_sample_references():
    rng = np.random.default_rng(5)
    f = rng.normal(size=int(np.prod(SIZES))).astype(F)
    o = rng.uniform(-2, 10, size=(300, 3)).astype(F)
    d = rng.normal(size=(300, 3)).astype(F)
    t, pos, nrm, sd = ref.raycast(f, SIZES, o, d, step=0.37, refine=5, side=ref.EITHER, t_min=-np.inf)
    hit = sd != 0
    assert hit.sum() > 100
    v, g = sample_reference.sample(f, SIZES, pos[hit], gradients=True)
    ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    assert np.array_equal(nrm[hit], g / ln[:, None]) and np.abs(v).max() < 0.05     # on the iso-level, up to the last interpolation
    assert (np.sign((nrm[hit] * d[hit]).sum(1)) == -sd[hit]).mean() > 0.95           # a front crossing runs against the gradient


def test_a_weight_mask_hides_the_crossing():
    f = plane_field()
    o, d = face_rays(8.0, -1.0)
    W = np.ones(SIZES[::-1], F)
    assert (ref.raycast(f, SIZES, o, d, weight=W)[0] == F(4.75)).all()
    W[:, :, 3] = 0.0                                  # the plane x = 3: the cells [2, 3] and [3, 4], across the crossing at 3.25
    t, pos, nrm, sd = ref.raycast(f, SIZES, o, d, weight=W)
    assert np.isposinf(t).all() and not sd.any()
    W[:, :, 3] = 0.5
    below, at = np.nextafter(F(0.5), F(1)), F(0.5)
    assert np.isposinf(ref.raycast(f, SIZES, o, d, weight=W, min_weight=below)[0]).all()     # W just below min_weight
    assert (ref.raycast(f, SIZES, o, d, weight=W, min_weight=at)[0] == F(4.75)).all()        # W just at it
    W[:, :, 3] = np.nan
    assert np.isposinf(ref.raycast(f, SIZES, o, d, weight=W)[0]).all()
    # a non-finite value ends a bracket the same way
    g = f.copy().reshape(SIZES[::-1])
    g[:, :, 4] = np.nan
    assert np.isposinf(ref.raycast(g, SIZES, o, d)[0]).all()


def sphere_figures(field, weight, **options):
    """the render of the sphere case against the exact image -> a dict of figures"""
    cam = cases.sphere_camera()
    exact, miss = cases.cast_balls(cam, cases.SPHERE)
    depth, pos, nrm, inc = ref.render(field, cases.SIZES, cam, weight=weight, **options)
    hit, true = np.isfinite(depth), np.isfinite(exact)
    interior = miss <= math.sqrt(10.0 ** 2 - 4.0)
    both = hit & interior                             # the figures are taken over the interior pixels
    err = np.abs(depth[both].astype(np.float64) - exact[both])
    lit = both & (inc > 0)
    radial = pos[lit].astype(np.float64) - cases.CENTRE
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    cos = (nrm[lit].astype(np.float64) * radial).sum(1)
    return {"true": int(true.sum()), "interior": int(interior.sum()), "interior_hit": int((interior & hit).sum()),
            "differ": int((hit != true).sum()), "extra": int((hit & ~true).sum()), "lost": int((true & ~hit).sum()),
            "rms": float(np.sqrt(np.mean(err ** 2))), "max": float(err.max()),
            "angle": float(np.degrees(np.arccos(np.clip(cos, -1, 1))).max()), "lit": int(lit.sum())}


# the restatement's own figures on the analytic sphere (32^3, r = 10, 96^2 range image), measured with the committed code on
# the CPU: |depth - exact| (rms, max) and the angle between the normal and the radius (degrees, max) over the 2 128 interior
# pixels, and the pixels of the 2 212-pixel silhouette that differ in hit or miss (all of them lost at the grazing rim)
SPHERE_FIGURES = {
    (1.0, 4): dict(rms=0.0321, max=0.1086, differ=14, angle=3.96),
    (1.0, 0): dict(rms=0.0439, max=0.1618, differ=14, angle=3.91),
    (0.5, 6): dict(rms=0.0321, max=0.1085, differ=6, angle=3.95),
    (2.0, 8): dict(rms=0.0321, max=0.1085, differ=20, angle=3.95),
}


@pytest.mark.parametrize("step,refine", sorted(SPHERE_FIGURES))
def test_the_analytic_sphere(step, refine):
    got = sphere_figures(cases.ball_field(cases.SPHERE), None, step=step, refine=refine)
    print("analytic sphere, step %g refine %d: %r" % (step, refine, got))
    want = SPHERE_FIGURES[(step, refine)]
    assert got["true"] == 2212 and got["interior"] == 2128
    assert got["interior_hit"] == got["interior"]                     # every ray that passes well inside the sphere hits
    assert got["max"] < 0.5                                           # no error reaches half a cell
    assert got["rms"] <= MARGIN * want["rms"] and got["max"] <= MARGIN * want["max"]
    assert got["differ"] <= MARGIN * want["differ"] and got["angle"] <= MARGIN * want["angle"]


# the same for the volume fused from 4.27's 14 views, rendered under its weight mask
FUSED_FIGURES = dict(rms=0.0376, max=0.1695, extra=4, lost=8, angle=6.31)


def test_the_fused_volume():
    t, W = cases.fused(cases.SPHERE)
    got = sphere_figures(t, W)
    print("fused sphere, step 1 refine 4: %r" % (got,))
    assert got["interior_hit"] == got["interior"] and got["max"] < 0.5
    assert got["rms"] <= MARGIN * FUSED_FIGURES["rms"] and got["max"] <= MARGIN * FUSED_FIGURES["max"]
    assert got["extra"] <= MARGIN * FUSED_FIGURES["extra"] and got["lost"] <= MARGIN * FUSED_FIGURES["lost"]
    assert got["angle"] <= MARGIN * FUSED_FIGURES["angle"]


def test_a_render_is_its_rays_and_feeds_the_depth_unit():
    cam = cases.sphere_camera(size=24, kind=dref.Z)
    f = cases.ball_field(cases.SPHERE)
    depth, pos, nrm, inc = ref.render(f, cases.SIZES, cam)
    o, d, px, py = ref.pixel_rays(cam)
    t, p2, n2, sd = ref.raycast(f, cases.SIZES, o, d)
    hit = sd != 0
    assert np.array_equal(depth[hit], t[hit]) and np.isposinf(depth[~hit]).all() and np.array_equal(pos, p2, equal_nan=True)
    assert np.array_equal(nrm, n2) and (inc[hit] > 0).all() and not inc[~hit].any()
    back, _, _, valid = dref.unproject(cam, depth)                     # +inf is "no depth" to the depth unit
    assert np.array_equal(valid.astype(bool), hit) and np.abs(back[hit] - pos[hit]).max() < 1e-3
    rng_img = ref.render(f, cases.SIZES, cases.sphere_camera(size=24, kind=dref.RANGE))[0]
    scale = np.sqrt((px * px + py * py) + F(1))
    assert np.array_equal(rng_img[hit], t[hit] * scale[hit])
    far = ref.render(f, cases.SIZES, cam, side=ref.BACK)                # a back hit faces away: no normal, no incidence
    assert np.isfinite(far[0]).sum() == hit.sum() and not far[2].any() and not far[3].any()


@pytest.mark.parametrize("degrees,scale", [(3.0, 1.0), (6.0, 2.0)])
def test_tracking_on_the_restatement_chain(degrees, scale):
    true, guess, errors, cam, total, log = cases.tracked(degrees, scale, 2)
    (a0, s0), (a1, s1), (a2, s2) = errors
    r = log[0]["registration"]
    print("tracking from %.2f deg / %.3f: round 1 %.4f deg / %.4f (%d steps, %d of %d pairs, %d rendered), round 2 %.4f deg / %.4f"
          % (a0, s0, a1, s1, r["iterations"], r["counted"], r["queries"], log[0]["rendered"], a2, s2))
    assert abs(a0 - degrees) < 1e-3 and abs(s0 - scale * math.sqrt(0.5)) < 1e-3
    assert a1 <= a0 / 5 and s1 <= s0 / 5                              # the first round divides both errors by at least 5
    assert a2 <= 2 * a1 and s2 <= 2 * s1                              # a second round does not undo it
    E = cases.rigid(guess) @ np.linalg.inv(total)                      # the correction is the product of the rounds' transforms
    assert np.abs(E[:3] - cases.rigid(cam)[:3]).max() < 1e-5
