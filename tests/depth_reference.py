"""The contract of the depth unit (include/fi_hip.h fi_depth_unproject, fi_volume_integrate, fi_volume_constraints; DESIGN.md
4.27) restated in numpy: fp32 elementwise, one rounding per operation, written for all pixels or all voxels at once.  The
device is held to these functions bit for bit (tests/test_gpu_depth.py); tests/test_depth_reference.py holds them to
geometry known by hand.  Only numpy."""
import math

import numpy as np

F = np.float32
Z, RANGE = 0, 1
CAMERAS = 8        # FI_DEPTH_CAMERAS: images per pass of the device kernel (no result depends on it)


class Cam:
    """fi_camera: pose (3, 4) float32 = [R | t], world to camera"""

    def __init__(self, pose, fx, fy, cx, cy, width, height, kind):
        self.pose = np.asarray(pose, F).reshape(3, 4)
        self.fx, self.fy, self.cx, self.cy = F(fx), F(fy), F(cx), F(cy)
        self.width, self.height, self.kind = int(width), int(height), int(kind)


def look_at(eye, target, up, fov_y, width, height, kind=RANGE):
    """camera_look_at: float64, rounded to float32 once"""
    eye = np.asarray(eye, np.float64).reshape(3)
    fwd = np.asarray(target, np.float64).reshape(3) - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.asarray(up, np.float64).reshape(3))
    right /= np.linalg.norm(right)
    top = np.cross(right, fwd)
    R = np.stack([right, -top, fwd])
    f = height / (2.0 * math.tan(0.5 * fov_y))
    return Cam(np.concatenate([R, -(R @ eye)[:, None]], axis=1), f, f, 0.5 * width, 0.5 * height, width, height, kind)


def _valid(d):
    return (d > 0) & (d < np.inf)


def _camera_points(cam, rows, cols, d):
    px = ((cols.astype(F) + F(0.5)) - cam.cx) / cam.fx
    py = ((rows.astype(F) + F(0.5)) - cam.cy) / cam.fy
    if cam.kind == Z:
        return px * d, py * d, d * F(1)
    ln = np.sqrt((px * px + py * py) + F(1))
    return (px / ln) * d, (py / ln) * d, (F(1) / ln) * d


def _rotate_back(cam, e):
    R = cam.pose[:, :3]
    return [(R[0, j] * e[0] + R[1, j] * e[1]) + R[2, j] * e[2] for j in range(3)]


def _world_points(cam, d):
    """the world point of every pixel of the (h, w) image d (garbage where d is not valid)"""
    rows, cols = np.meshgrid(np.arange(cam.height), np.arange(cam.width), indexing="ij")
    c = _camera_points(cam, rows, cols, d)
    t = cam.pose[:, 3]
    return np.stack(_rotate_back(cam, [c[a] - t[a] for a in range(3)]), axis=-1), c


def _shift(a, drow, dcol, fill):
    """out[r, c] = a[r + drow, c + dcol], `fill` outside the image"""
    out = np.full_like(a, fill)
    h, w = a.shape[:2]
    rs, cs = slice(max(0, -drow), min(h, h - drow)), slice(max(0, -dcol), min(w, w - dcol))
    rd, cd = slice(max(0, drow), min(h, h + drow)), slice(max(0, dcol), min(w, w + dcol))
    out[rs, cs] = a[rd, cd]
    return out


def _difference(P, d, ok, drow, dcol, max_jump):
    """(difference (h, w, 3), has (h, w)) along one image axis: after minus before, central or one-sided"""
    out, has = [], []
    for sign in (+1, -1):
        dn = _shift(d, sign * drow, sign * dcol, F(0))
        okn = _shift(ok, sign * drow, sign * dcol, False)
        has.append(okn & (np.abs(dn - d) <= max_jump))
        out.append(_shift(P, sign * drow, sign * dcol, F(0)))
    after = np.where(has[0][..., None], out[0], P)
    before = np.where(has[1][..., None], out[1], P)
    return after - before, has[0] | has[1]


def unproject(cam, depth, max_jump=np.inf):
    """fi_depth_unproject -> positions (h w, 3), normals (h w, 3), incidence (h w,) float32, valid (h w,) uint8"""
    d = np.asarray(depth, F).reshape(cam.height, cam.width)
    max_jump = F(max_jump)
    with np.errstate(all="ignore"):
        ok = _valid(d)
        P, c = _world_points(cam, d)
        a, has_a = _difference(P, d, ok, 0, 1, max_jump)
        b, has_b = _difference(P, d, ok, 1, 0, max_jump)
        n = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                      a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)
        ln = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
        n = n / ln[..., None]
        v = _rotate_back(cam, c)
        lv = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        s = (n[..., 0] * (v[0] / lv) + n[..., 1] * (v[1] / lv)) + n[..., 2] * (v[2] / lv)
        flip = s > 0
        n = np.where(flip[..., None], -n, n)
        s = np.where(flip, -s, s)
        q = -s
        q = np.where(q < 1, q, F(1))
        has = ok & has_a & has_b & (ln > 0) & (ln < np.inf) & (q > 0)
    positions = np.where(ok[..., None], P, F(np.nan)).astype(F)
    normals = np.where(has[..., None], n, F(0)).astype(F)
    incidence = np.where(has, q, F(0)).astype(F)
    return positions.reshape(-1, 3), normals.reshape(-1, 3), incidence.reshape(-1), ok.reshape(-1).astype(np.uint8)


def voxel_coordinates(sizes):
    """(X, Y, Z) float32 of every voxel, x fastest"""
    k, j, i = np.meshgrid(np.arange(sizes[2]), np.arange(sizes[1]), np.arange(sizes[0]), indexing="ij")
    return i.reshape(-1).astype(F), j.reshape(-1).astype(F), k.reshape(-1).astype(F)


def integrate(sizes, truncation, max_weight, tsdf, weight, cams, depths, incidences=None, image_weights=None, min_incidence=0.5):
    """fi_volume_integrate on the state (tsdf, weight) -> the new (tsdf, weight).  depths / incidences: one image per camera."""
    X, Y, Zc = voxel_coordinates(sizes)
    t, W = np.array(tsdf, F).reshape(-1), np.array(weight, F).reshape(-1)
    truncation, max_weight, min_incidence = F(truncation), F(max_weight), F(min_incidence)
    with np.errstate(all="ignore"):
        for s, cam in enumerate(cams):
            d_img = np.asarray(depths[s], F).reshape(-1)
            p = cam.pose
            cx = ((p[0, 0] * X + p[0, 1] * Y) + p[0, 2] * Zc) + p[0, 3]
            cy = ((p[1, 0] * X + p[1, 1] * Y) + p[1, 2] * Zc) + p[1, 3]
            cz = ((p[2, 0] * X + p[2, 1] * Y) + p[2, 2] * Zc) + p[2, 3]
            go = cz > 0
            fu = np.floor(cam.fx * (cx / cz) + cam.cx)
            fv = np.floor(cam.fy * (cy / cz) + cam.cy)
            go &= (fu >= 0) & (fu < F(2147483648.0)) & (fv >= 0) & (fv < F(2147483648.0))
            col = np.where(go, fu, 0).astype(np.int64)
            row = np.where(go, fv, 0).astype(np.int64)
            go &= (col < cam.width) & (row < cam.height)
            pix = np.where(go, row * cam.width + col, 0)
            d = d_img[pix]
            go &= _valid(d)
            r = cz if cam.kind == Z else np.sqrt((cx * cx + cy * cy) + cz * cz)
            e = d - r
            go &= ~(e < -truncation)
            q = np.ones_like(d)
            if incidences is not None:
                q = np.asarray(incidences[s], F).reshape(-1)[pix]
                go &= (q >= min_incidence) & (np.abs(q) < np.inf)
            g = (e * q) / truncation
            f = np.where(g < 1, g, F(1))
            w = q * (F(1) if image_weights is None else F(image_weights[s]))
            go &= w > 0
            total = W + w
            t = np.where(go, (t * W + f * w) / total, t).astype(F)
            W = np.where(go, np.where(total < max_weight, total, max_weight), W).astype(F)
    return t, W


def fresh(sizes):
    n = int(np.prod(sizes))
    return np.ones(n, F), np.zeros(n, F)


def constraints(sizes, truncation, max_weight, tsdf, weight, min_weight=0.0):
    """fi_volume_constraints -> positions (n, 3), values (n,), weights (n,) float32"""
    t, W = np.asarray(tsdf, F).reshape(-1), np.asarray(weight, F).reshape(-1)
    with np.errstate(all="ignore"):
        band = (W >= F(min_weight)) & (W > 0) & (np.abs(t) < 1)
    X, Y, Zc = voxel_coordinates(sizes)
    return (np.stack([X[band], Y[band], Zc[band]], axis=1), (t[band] * F(truncation)).astype(F), (W[band] / F(max_weight)).astype(F))
