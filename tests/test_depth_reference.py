"""tests/depth_reference.py, the numpy definition of the depth unit's contract, held to geometry known by hand: the camera of
camera_look_at against SurfaceIndex.render_depth's ray formula, unprojected planes and spheres against their surfaces, and
the fusion of 14 views of a sphere against the true distance.  No GPU: the device is held to the same functions bit for bit
in tests/test_gpu_depth.py."""
import math

import numpy as np
import pytest

import depth_reference as ref
from field_interpolation_amd import Camera, camera_look_at

F = np.float32
CENTRE = np.array([15.5, 15.5, 15.5])
RADIUS = 10.0
FOV = math.radians(50.0)


def eyes(distance=40.0):
    """6 axis and 8 diagonal viewpoints around CENTRE"""
    dirs = [np.eye(3)[a] * s for a in range(3) for s in (1, -1)]
    dirs += [np.array([sx, sy, sz]) / math.sqrt(3.0) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    return [CENTRE + distance * d for d in dirs]


def up_for(eye):
    return (0.0, 0.0, 1.0) if abs((eye - CENTRE)[2]) < 0.9 * np.linalg.norm(eye - CENTRE) else (0.0, 1.0, 0.0)


def rays(cam):
    """(eye (3,), unit directions (h, w, 3), cosine to the optical axis (h, w)) in float64"""
    R, t = cam.pose[:, :3].astype(np.float64), cam.pose[:, 3].astype(np.float64)
    rows, cols = np.meshgrid(np.arange(cam.height), np.arange(cam.width), indexing="ij")
    d = np.stack([(cols + 0.5 - cam.cx) / cam.fx, (rows + 0.5 - cam.cy) / cam.fy, np.ones(rows.shape)], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return -R.T @ t, d @ R, d[..., 2]


def cast_sphere(cam, centre=CENTRE, radius=RADIUS):
    """the depth image of a sphere in the camera's kind, +inf where the ray misses"""
    eye, d, cos = rays(cam)
    oc = eye - centre
    b = d @ oc
    disc = b * b - (oc @ oc - radius * radius)
    t = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), np.inf)
    t = np.where(t > 0, t, np.inf)
    return (t * (cos if cam.kind == ref.Z else 1.0)).astype(F)


def cast_plane(cam, normal, offset):
    """the depth image of the plane normal . x = offset"""
    eye, d, cos = rays(cam)
    den = d @ normal
    t = np.where(np.abs(den) > 1e-9, (offset - eye @ normal) / np.where(den == 0, 1, den), np.inf)
    t = np.where(t > 0, t, np.inf)
    return (t * (cos if cam.kind == ref.Z else 1.0)).astype(F)


def test_camera_look_at_has_render_depths_rays():
    eye, target, up, width, height = np.array([50.0, -7.0, 21.0]), CENTRE, (0.0, 0.0, 1.0), 33, 17
    cam = camera_look_at(eye, target, up, FOV, width, height)
    assert isinstance(cam, Camera) and cam.kind == "range" and (cam.width, cam.height) == (width, height)
    mine = ref.look_at(eye, target, up, FOV, width, height)
    assert np.array_equal(cam.pose, mine.pose) and (F(cam.fx), F(cam.cx), F(cam.cy)) == (mine.fx, mine.cx, mine.cy)
    # SurfaceIndex.render_depth's direction formula, restated
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.asarray(up))
    right /= np.linalg.norm(right)
    top = np.cross(right, fwd)
    h = math.tan(0.5 * FOV)
    x = ((np.arange(width) + 0.5) / width * 2 - 1) * h * width / height
    y = (1 - (np.arange(height) + 0.5) / height * 2) * h
    want = fwd[None, None, :] + x[None, :, None] * right[None, None, :] + y[:, None, None] * top[None, None, :]
    want /= np.linalg.norm(want, axis=2, keepdims=True)
    got_eye, got, _ = rays(mine)
    # the camera is rounded to float32 once: 2^-24 relative on each of R, fx, cx, and on t against coordinates of 50
    assert np.abs(got - want).max() < 8 * 2.0 ** -24
    assert np.abs(got_eye - eye).max() < 50 * 8 * 2.0 ** -24


@pytest.mark.parametrize("kind", [ref.RANGE, ref.Z])
def test_unprojected_plane_and_sphere_lie_on_their_surfaces(kind):
    cam = ref.look_at(eyes()[6], CENTRE, up_for(eyes()[6]), FOV, 96, 96, kind)
    # a plane through the centre, tilted 30 degrees against the view: no jumps, every pixel valid
    n = CENTRE - eyes()[6]
    n /= np.linalg.norm(n)
    n = n + 0.5 * np.cross(n, [0.0, 0.0, 1.0])
    n /= np.linalg.norm(n)
    pos, nrm, inc, valid = ref.unproject(cam, cast_plane(cam, n, n @ CENTRE))
    assert valid.all() and np.abs(pos.astype(np.float64) @ n - n @ CENTRE).max() < 1e-4   # float32 depth at range 60: 4e-6 a step
    assert (inc > 0).all() and np.abs(np.abs(nrm.astype(np.float64) @ n) - 1).max() < 1e-5   # differences within the plane
    assert (nrm.astype(np.float64) @ (eyes()[6] - CENTRE) > 0).all()                          # towards the eye
    # the sphere: a silhouette, invalid pixels around it
    depth = cast_sphere(cam)
    pos, nrm, inc, valid = ref.unproject(cam, depth)
    ok = valid.astype(bool)
    assert 0 < ok.sum() < ok.size and np.isnan(pos[~ok]).all() and not nrm[~ok].any() and not inc[~ok].any()
    rel = pos[ok].astype(np.float64) - CENTRE
    assert np.abs(np.linalg.norm(rel, axis=1) - RADIUS).max() < 1e-4
    # normals, away from the silhouette (incidence >= 0.5 and the four neighbours valid): two neighbours lie at most
    # 2 * 0.29 / 0.5 = 1.2 lattice units apart on the sphere (the pixel's footprint at range 30, stretched by the
    # incidence), a chord that subtends 0.116 rad of it; the chord's normal is within half of that of the true one
    # however unevenly the pixel divides it: 0.058 rad = 3.4 degrees
    v = ok.reshape(96, 96)
    inner = np.zeros_like(v)
    inner[1:-1, 1:-1] = v[1:-1, 1:-1] & v[:-2, 1:-1] & v[2:, 1:-1] & v[1:-1, :-2] & v[1:-1, 2:]
    pick = inner.reshape(-1) & (inc >= 0.5)
    true = (pos[pick].astype(np.float64) - CENTRE) / RADIUS
    cos = (nrm[pick].astype(np.float64) * true).sum(1)
    print("sphere normals: %d pixels, worst angle %.3f degrees" % (pick.sum(), np.degrees(np.arccos(cos.min()))))
    assert pick.sum() > 1000 and np.degrees(np.arccos(np.clip(cos, -1, 1))).max() < 3.4
    # the incidence is the cosine between the normal and the ray back to the eye
    back = eyes()[6] - pos[pick].astype(np.float64)
    back /= np.linalg.norm(back, axis=1, keepdims=True)
    assert np.abs((nrm[pick].astype(np.float64) * back).sum(1) - inc[pick]).max() < 1e-5


def test_depth_jumps_take_one_sided_differences():
    cam = ref.look_at(eyes()[0], CENTRE, up_for(eyes()[0]), FOV, 33, 17, ref.Z)
    depth = np.full((17, 33), 30.0, F)
    depth[:, 16:] = 50.0                    # two fronto-parallel planes, a jump of 20 between columns 15 and 16
    pos, nrm, inc, valid = ref.unproject(cam, depth, max_jump=1.0)
    axis = (CENTRE - eyes()[0]) / 40.0
    assert valid.all() and np.abs(np.abs(nrm.astype(np.float64) @ axis) - 1).max() < 1e-5    # one-sided: still the planes' normal
    _, tilted, _, _ = ref.unproject(cam, depth)                                          # any jump allowed: the edge pixels tilt
    edge = np.zeros((17, 33), bool)
    edge[:, 15:17] = True
    assert (np.abs(tilted[edge.reshape(-1)].astype(np.float64) @ axis) < 0.5).all()
    assert np.array_equal(tilted[~edge.reshape(-1)], nrm[~edge.reshape(-1)])
    depth[:, 15] = np.nan                   # a pixel between two others that do not qualify has no normal
    depth[:, 17] = -1.0
    pos, nrm, inc, valid = ref.unproject(cam, depth, max_jump=1.0)
    lone = np.zeros((17, 33), bool)
    lone[:, 16] = True
    assert valid[lone.reshape(-1)].all() and not nrm[lone.reshape(-1)].any() and not inc[lone.reshape(-1)].any()
    assert np.isfinite(pos[lone.reshape(-1)]).all() and not valid.reshape(17, 33)[:, 15].any() and not valid.reshape(17, 33)[:, 17].any()


def sphere_views(size=96, kind=ref.RANGE):
    cams = [ref.look_at(e, CENTRE, up_for(e), FOV, size, size, kind) for e in eyes()]
    depths = [cast_sphere(c) for c in cams]
    incs = [ref.unproject(c, d)[2] for c, d in zip(cams, depths)]
    return cams, depths, incs


def fusion_errors(tsdf, weight, truncation):
    X, Y, Z = ref.voxel_coordinates([32, 32, 32])
    true = np.linalg.norm(np.stack([X, Y, Z], 1).astype(np.float64) - CENTRE, axis=1) - RADIUS
    band = (weight > 0) & (np.abs(tsdf) < 1)
    est = tsdf.astype(np.float64) * truncation
    near = np.abs(true) <= 1.0
    return true, band, math.sqrt(np.mean((est - true)[near & band] ** 2)), np.abs(est - true)[near & band].max(), (near & ~band).sum()


def test_fusing_14_views_of_a_sphere_gives_its_distance():
    sizes, truncation = [32, 32, 32], 3.0
    cams, depths, incs = sphere_views()
    t, W = ref.integrate(sizes, truncation, 64.0, *ref.fresh(sizes), cams, depths, incs, min_incidence=0.5)
    true, band, rms, worst, missing = fusion_errors(t, W, truncation)
    t0, W0 = ref.integrate(sizes, truncation, 64.0, *ref.fresh(sizes), cams, depths)
    _, _, rms0, worst0, _ = fusion_errors(t0, W0, truncation)
    print("sphere fusion, 14 views: with the image incidences rms %.4f max %.4f; plain projective rule rms %.4f max %.4f"
          % (rms, worst, rms0, worst0))
    assert band[np.abs(true) <= 0.5].all()                                # every voxel within 0.5 of the surface is in the band
    far = band & (np.abs(true) > 0.25)
    assert (np.sign(t[far]) == np.sign(true[far])).all()                  # the sign, beyond 0.25
    assert missing == 0 and rms < 0.25                                    # a quarter cell


def small_case():
    sizes = [12, 10, 9]
    centre = np.array([5.5, 4.5, 4.0])
    cam = ref.look_at(centre + [0.0, 0.0, 25.0], centre, (0.0, 1.0, 0.0), math.radians(40.0), 24, 20, ref.Z)
    return sizes, cam, np.full((20, 24), 25.0, F)        # a wall through the middle plane z = 4


def test_max_weight_clamps_and_a_zero_image_weight_changes_nothing():
    sizes, cam, depth = small_case()
    t, W = ref.fresh(sizes)
    for _ in range(5):
        t, W = ref.integrate(sizes, 2.0, 3.0, t, W, [cam], [depth])
    assert W.max() == 3.0 and set(np.unique(W)) <= {0.0, 3.0}
    t2, W2 = ref.integrate(sizes, 2.0, 3.0, t, W, [cam], [depth * 0.5], image_weights=[0.0])
    assert np.array_equal(t2, t) and np.array_equal(W2, W)
    t3, W3 = ref.integrate(sizes, 2.0, 3.0, t, W, [cam], [depth * F(1.02)], image_weights=[2.0])
    assert not np.array_equal(t3, t) and W3.max() == 3.0


def test_image_order_matters_only_through_the_rule():
    sizes, cam, depth = small_case()
    near, far = depth - F(0.5), depth + F(0.5)
    a = ref.integrate(sizes, 2.0, 0.75, *ref.fresh(sizes), [cam, cam], [near, far])      # the clamp at 0.75 bites at the first
    b = ref.integrate(sizes, 2.0, 0.75, *ref.fresh(sizes), [cam, cam], [far, near])
    assert not np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    one = ref.integrate(sizes, 2.0, 0.75, *ref.fresh(sizes), [cam], [near])
    two = ref.integrate(sizes, 2.0, 0.75, *one, [cam], [far])
    assert np.array_equal(two[0], a[0]) and np.array_equal(two[1], a[1])                 # two calls = one call over both
    # by hand at a seen voxel: the first image leaves (f1, 0.75), the second (f1 * 0.75 + f2 * 1) / 1.75 and the clamp again
    other = ref.integrate(sizes, 2.0, 0.75, *ref.fresh(sizes), [cam], [far])
    i = int(np.flatnonzero((one[1] > 0) & (other[1] > 0))[0])
    f1, f2 = one[0][i], other[0][i]
    assert a[0][i] == (F(f1) * F(0.75) + F(f2) * F(1)) / F(1.75) and a[1][i] == F(0.75)


def test_bad_depths_are_skipped_and_a_camera_inside_skips_what_is_behind_it():
    sizes, cam, depth = small_case()
    bad = depth.copy()
    bad[:5], bad[5:10], bad[10:15], bad[15:] = np.nan, np.inf, 0.0, -3.0
    t, W = ref.integrate(sizes, 2.0, 64.0, *ref.fresh(sizes), [cam], [bad])
    assert np.array_equal(t, np.ones_like(t)) and not W.any()
    inside = ref.look_at([5.5, 4.5, 4.0], [5.5, 4.5, 30.0], (0.0, 1.0, 0.0), math.radians(90.0), 24, 20, ref.RANGE)
    t, W = ref.integrate(sizes, 2.0, 64.0, *ref.fresh(sizes), [inside], [np.full((20, 24), 3.0, F)])
    Wz = W.reshape(9, 10, 12)
    assert not Wz[:5].any() and Wz[5:].any()              # z <= 4: at or behind the eye; in front: seen
    p, v, w = ref.constraints(sizes, 2.0, 64.0, t, W)
    assert len(p) == len(v) == len(w) > 0 and (p[:, 2] >= 5).all() and (np.abs(v) < 2.0).all() and (w == F(1) / F(64)).all()
    assert len(ref.constraints(sizes, 2.0, 64.0, t, W, min_weight=2.0)[0]) == 0
