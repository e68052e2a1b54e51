"""Cases the march tests share (tests/test_march_reference.py, tests/test_gpu_march.py): unions of balls at 32^3 as analytic
fields, as exact depth images and as volumes fused from 14 views, and the tracking case of DESIGN.md 4.28.  Every case is
computed once per process and handed out unchanged.  Only numpy and the restatements."""
import functools
import math

import numpy as np

import depth_reference as dref
import march_reference as mref
import register_reference as rref

F = np.float32
SIZES = [32, 32, 32]
CENTRE = np.array([15.5, 15.5, 15.5])
FOV = math.radians(50.0)
TRUNCATION = 3.0
SPHERE = ((15.5, 15.5, 15.5, 10.0),)
THREE = ((14.0, 15.0, 15.0, 8.0), (21.0, 19.0, 14.0, 5.0), (12.0, 22.0, 19.0, 4.0))


def eyes(distance=40.0):
    """4.27's 6 axis and 8 diagonal viewpoints around CENTRE"""
    dirs = [np.eye(3)[a] * s for a in range(3) for s in (1, -1)]
    dirs += [np.array([sx, sy, sz]) / math.sqrt(3.0) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    return [CENTRE + distance * d for d in dirs]


def up_for(eye):
    return (0.0, 0.0, 1.0) if abs((eye - CENTRE)[2]) < 0.9 * np.linalg.norm(eye - CENTRE) else (0.0, 1.0, 0.0)


def rays(cam):
    """(eye (3,), unit directions (h w, 3), cosine to the optical axis (h w,)) in float64"""
    R, t = cam.pose[:, :3].astype(np.float64), cam.pose[:, 3].astype(np.float64)
    rows, cols = np.meshgrid(np.arange(cam.height), np.arange(cam.width), indexing="ij")
    d = np.stack([(cols + 0.5 - cam.cx) / cam.fx, (rows + 0.5 - cam.cy) / cam.fy, np.ones(rows.shape)], axis=-1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return -R.T @ t, d @ R, d[:, 2]


def cast_balls(cam, balls):
    """(the exact depth image (h w,) float64 of a union of balls in the camera's kind, +inf where the ray misses; the closest
    approach of each ray to the first ball's centre)"""
    eye, d, cos = rays(cam)
    best = np.full(len(d), np.inf)
    for x, y, z, r in balls:
        oc = eye - np.array([x, y, z])
        b = d @ oc
        disc = b * b - (oc @ oc - r * r)
        t = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), np.inf)
        best = np.minimum(best, np.where(t > 0, t, np.inf))
    oc = eye - np.array(balls[0][:3])
    miss = np.sqrt(np.maximum(oc @ oc - (d @ oc) ** 2, 0.0))
    return best * (cos if cam.kind == dref.Z else 1.0), miss


@functools.lru_cache(maxsize=None)
def ball_field(balls):
    """f = min over the balls of |x - c| - r at every point of SIZES, float32, x fastest"""
    X, Y, Z = dref.voxel_coordinates(SIZES)
    p = np.stack([X, Y, Z], 1).astype(np.float64)
    f = np.min([np.linalg.norm(p - np.array(b[:3]), axis=1) - b[3] for b in balls], axis=0).astype(F)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def fused(balls):
    """(tsdf, weight) of the balls fused from the 14 views at 96^2, truncation 3, image incidences"""
    cams = [dref.look_at(e, CENTRE, up_for(e), FOV, 96, 96, dref.RANGE) for e in eyes()]
    depths = [cast_balls(c, balls)[0].astype(F) for c in cams]
    incs = [dref.unproject(c, d)[2] for c, d in zip(cams, depths)]
    t, W = dref.integrate(SIZES, TRUNCATION, 64.0, *dref.fresh(SIZES), cams, depths, incs, min_incidence=0.5)
    t.setflags(write=False)
    W.setflags(write=False)
    return t, W


def sphere_camera(size=96, kind=dref.RANGE):
    eye = CENTRE + np.array([24.0, 0.0, 32.0])
    return dref.look_at(eye, CENTRE, up_for(eye), FOV, size, size, kind)


def rotation(axis, degrees):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = math.radians(degrees)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def rigid(cam):
    G = np.eye(4)
    G[:3] = cam.pose.astype(np.float64)
    return G


def tracking_case(degrees=3.0, shift=(0.5, -0.4, 0.3)):
    """(the true camera, its exact 48^2 depth image of THREE, the guessed camera): the guess is the true camera carried along
    by a turn of `degrees` about (0.3, 1, 0.2) through CENTRE and the shift"""
    u = np.array([0.5, 0.3, 0.81])
    eye = CENTRE + 38.0 * u / np.linalg.norm(u)
    true = dref.look_at(eye, CENTRE + np.array([1.0, -0.5, 0.5]), up_for(eye), FOV, 48, 48, dref.RANGE)
    depth = cast_balls(true, THREE)[0].astype(F)
    M = np.eye(4)
    M[:3, :3] = rotation([0.3, 1.0, 0.2], degrees)
    M[:3, 3] = CENTRE - M[:3, :3] @ CENTRE + np.asarray(shift, np.float64)
    G = rigid(true) @ np.linalg.inv(M)
    return true, depth, dref.Cam(G[:3].astype(F), true.fx, true.fy, true.cx, true.cy, 48, 48, true.kind)


def pose_errors(true, cam):
    """(the rotation between the two poses in degrees, the displacement of CENTRE between them)"""
    E = np.linalg.inv(rigid(cam)) @ rigid(true)
    angle = math.degrees(math.acos(min(1.0, max(-1.0, 0.5 * (np.trace(E[:3, :3]) - 1.0)))))
    return angle, float(np.linalg.norm(E[:3, :3] @ CENTRE + E[:3, 3] - CENTRE))


def reference_register(source, target, normals, mode="plane", max_distance=np.inf, **keywords):
    assert mode == "plane"
    return rref.register(rref.Target(points=target, normals=normals), source, mode=rref.PLANE, max_distance=max_distance, **keywords)


@functools.lru_cache(maxsize=None)
def tracked(degrees=3.0, scale=1.0, rounds=2):
    """march_reference.track of the tracking case on the restatement chain -> (true camera, guess, per-round cameras' errors,
    the final camera, the correction, the log)"""
    true, depth, guess = tracking_case(degrees, tuple(scale * s for s in (0.5, -0.4, 0.3)))
    t, W = fused(THREE)
    errors, cam = [pose_errors(true, guess)], guess
    total, log = np.eye(4), []
    for _ in range(rounds):
        cam, T, lg = mref.track(t, W, SIZES, TRUNCATION, cam, depth, reference_register, rounds=1)
        total = T @ total
        log += lg
        errors.append(pose_errors(true, cam))
    return true, guess, errors, cam, total, log
