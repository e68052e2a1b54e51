"""The contract of the colour unit (include/fi_hip.h fi_volume_integrate_colour, fi_volume_colour_sample,
fi_volume_render_colour, fi_volume_colour_constraints) restated in numpy: fp32 elementwise, one rounding per
operation, written for all voxels or all points at once.  The device is held to these functions bit for bit
(tests/test_gpu_colour.py); tests/test_colour_reference.py holds them to cases known by hand and holds the geometry half of
integrate_colour to depth_reference.integrate.  Only numpy."""
import numpy as np

import depth_reference
import march_reference

F = np.float32


def fresh(sizes, channels):
    """the colour state of a new volume: (channels, nvox) zeros and (nvox,) zeros"""
    n = int(np.prod(sizes))
    return np.zeros((channels, n), F), np.zeros(n, F)


def integrate_colour(sizes, truncation, max_weight, tsdf, weight, colour, colour_weight, cams, depths, colours, incidences=None,
                     image_weights=None, min_incidence=0.5, band=1.0):
    """fi_volume_integrate_colour on the state (tsdf, weight, colour (C, nvox), colour_weight) -> the new four arrays.
    depths / incidences: one image per camera; colours: one (h, w, C) image per camera.  Steps 1 - 8 are
    depth_reference.integrate's, statement for statement; steps 9 - 11 follow them."""
    X, Y, Zc = depth_reference.voxel_coordinates(sizes)
    t, W = np.array(tsdf, F).reshape(-1), np.array(weight, F).reshape(-1)
    Wc = np.array(colour_weight, F).reshape(-1)
    A = np.array(colour, F).reshape(-1, t.size)
    C = A.shape[0]
    truncation, max_weight, min_incidence, band = F(truncation), F(max_weight), F(min_incidence), F(band)
    with np.errstate(all="ignore"):
        for s, cam in enumerate(cams):
            d_img = np.asarray(depths[s], F).reshape(-1)
            c_img = np.asarray(colours[s], F).reshape(-1, C)
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
            go &= (d > 0) & (d < np.inf)
            r = cz if cam.kind == depth_reference.Z else np.sqrt((cx * cx + cy * cy) + cz * cz)
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
            # 9 - 11
            c = c_img[pix]                                              # (nvox, C)
            paint = go & (np.abs(g) < band) & (np.abs(c) < np.inf).all(axis=1)
            total = Wc + w
            for k in range(C):
                A[k] = np.where(paint, (A[k] * Wc + c[:, k] * w) / total, A[k]).astype(F)
            Wc = np.where(paint, np.where(total < max_weight, total, max_weight), Wc).astype(F)
    return t, W, A, Wc


def sample(sizes, colour, colour_weight, positions, min_weight=0.0):
    """fi_volume_colour_sample -> colours (n, C) float32, valid (n,) uint8"""
    nx, ny, nz = (int(s) for s in sizes)
    A = np.asarray(colour, F).reshape(-1, nx * ny * nz)
    Wc = np.asarray(colour_weight, F).reshape(-1)
    C = A.shape[0]
    P = np.asarray(positions, F).reshape(-1, 3)
    n = len(P)
    min_weight = F(min_weight)
    with np.errstate(all="ignore"):
        inside = np.ones(n, bool)
        cell, wts = [], []
        for j, size in enumerate((nx, ny, nz)):
            p = P[:, j]
            inside &= (p >= 0) & (p <= F(size - 1))                     # (a NaN fails both)
            fl, top = np.floor(p), F(size - 2)
            cf = np.where(fl < top, fl, top).astype(F)
            t = (p - cf).astype(F)
            cell.append(np.where(inside, cf, 0).astype(np.int64))
            wts.append(((F(1) - t).astype(F), t))
        S = np.zeros(n, F)
        N = np.zeros((n, C), F)
        for corner in range(8):
            a, b, c = corner & 1, (corner >> 1) & 1, corner >> 2
            omega = ((wts[0][a] * wts[1][b]) * wts[2][c]).astype(F)
            idx = ((cell[2] + c) * ny + (cell[1] + b)) * nx + (cell[0] + a)
            idx = np.where(inside, idx, 0)
            w = Wc[idx]
            counts = inside & (w > 0) & (w >= min_weight)
            S = np.where(counts, S + omega, S).astype(F)
            for k in range(C):
                N[:, k] = np.where(counts, N[:, k] + omega * A[k][idx], N[:, k])
        ok = S > 0
        out = np.where(ok[:, None], N / S[:, None], F(np.nan)).astype(F)
    return out, ok.astype(np.uint8)


def render_colour(sizes, tsdf, weight, colour, colour_weight, cam, step=1.0, refine=4, min_weight=0.0, colour_min_weight=0.0):
    """fi_volume_render_colour -> depth (h w,), positions (h w, 3), normals (h w, 3), incidence (h w,), colours (h w, C)"""
    depth, pos, nrm, inc = march_reference.render(tsdf, sizes, cam, 0.0, step, refine, march_reference.FRONT, weight, min_weight)
    return depth, pos, nrm, inc, sample(sizes, colour, colour_weight, pos, colour_min_weight)[0]


def constraints(sizes, max_weight, colour, colour_weight, min_weight=0.0):
    """fi_volume_colour_constraints -> positions (n, 3), colours (n, C), weights (n,) float32"""
    Wc = np.asarray(colour_weight, F).reshape(-1)
    A = np.asarray(colour, F).reshape(-1, Wc.size)
    with np.errstate(all="ignore"):
        keep = (Wc > 0) & (Wc >= F(min_weight))
    X, Y, Zc = depth_reference.voxel_coordinates(sizes)
    return (np.stack([X[keep], Y[keep], Zc[keep]], axis=1), np.ascontiguousarray(A[:, keep].T), (Wc[keep] / F(max_weight)).astype(F))
