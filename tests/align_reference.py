"""Numpy restatement of the contract of fi_align_correspondences (include/fi_hip.h): the rotation and shift
that most matched pairs of two point clouds agree on, by RANSAC with an exact inlier count.  Test infrastructure, independent
of the device code.  Every floating-point step is written the way the contract states it -- fp64 from the fp32 coordinates,
one rounding per operation, every sum in its stated order -- so that the mask and every figure returned are the bytes the
device must produce.  Only numpy and meshpts_reference.uniform / tree_sum."""
import numpy as np

from meshpts_reference import tree_sum, uniform
from plane_reference import confident as plane_confident

BATCH = 16384
SLICE = 256          # hypotheses scored at a time (memory only)


class Invalid(Exception):
    """what the device answers with FI_ERR_INVALID"""


class Unsupported(Exception):
    """what the device answers with FI_ERR_UNSUPPORTED"""


def check(n_s, n_t, m, threshold, similarity, max_trials, confidence):
    thr, sim = np.float32(threshold), np.float32(similarity)
    if n_s < 0 or n_t < 0 or m < 0:
        raise Invalid("counts")
    if not thr >= 0:
        raise Invalid("threshold")
    if not 0 <= sim <= 1:
        raise Invalid("similarity")
    if not 0.0 <= confidence < 1.0:
        raise Invalid("confidence")
    if not 1 <= max_trials <= 2 ** 31 - 1:
        raise Invalid("max_trials")
    if max(n_s, n_t, m) >= 2 ** 31:
        raise Unsupported("counts")


def nothing(pairs=0, live=0, trials=0, valid=0):
    return {"found": 0, "pairs": pairs, "live": live, "trials": trials, "valid": valid, "inliers": 0, "transform": np.eye(4), "rms": 0.0}


def squares(x):
    return (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2]


def cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], axis=-1)


def frame(p):
    """(e (k, 3, 3): e_1, e_2, e_3 as rows, ok (k,)) of the triangles p (k, 3, 3)"""
    u, w = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    l1 = np.sqrt(squares(u))
    e1 = u / l1[:, None]
    g = cross(e1, w)
    l = np.sqrt(squares(g))
    e3 = g / l[:, None]
    e2 = cross(e3, e1)
    return np.stack([e1, e2, e3], axis=1), np.isfinite(l1) & (l1 > 0.0) & np.isfinite(l) & (l > 0.0)


def hypotheses(X, Y, seed, h, similarity=0.0):
    """(R (k, 3, 3), t (k, 3), valid (k,)) of the hypotheses h (k,) over the live pairs' float64 points X -> Y (live, 3)"""
    live = len(X)
    h = np.asarray(h, np.uint64)
    j = [np.minimum(np.floor(uniform(seed, h * np.uint64(3) + np.uint64(k)) * np.float64(live)).astype(np.int64), live - 1)
         for k in range(3)]
    valid = (j[0] != j[1]) & (j[0] != j[2]) & (j[1] != j[2])
    a = np.stack([X[j[k]] for k in range(3)], axis=1)
    b = np.stack([Y[j[k]] for k in range(3)], axis=1)
    sim = np.float64(np.float32(similarity))
    with np.errstate(all="ignore"):
        if sim > 0:
            for p, q in ((0, 1), (0, 2), (1, 2)):
                ls, lt = squares(a[:, q] - a[:, p]), squares(b[:, q] - b[:, p])
                valid &= np.minimum(ls, lt) >= (sim * sim) * np.maximum(ls, lt)
        e, ok = frame(a)
        valid &= ok
        f, ok = frame(b)
        valid &= ok
        R = np.empty((len(h), 3, 3))
        for r in range(3):
            for c in range(3):
                R[:, r, c] = (f[:, 0, r] * e[:, 0, c] + f[:, 1, r] * e[:, 1, c]) + f[:, 2, r] * e[:, 2, c]
        cs = ((a[:, 0] + a[:, 1]) + a[:, 2]) / np.float64(3.0)
        ct = ((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float64(3.0)
        t = np.stack([ct[:, r] - ((R[:, r, 0] * cs[:, 0] + R[:, r, 1] * cs[:, 1]) + R[:, r, 2] * cs[:, 2]) for r in range(3)], axis=1)
    return R, t, valid


def misses(X, Y, R, t):
    """(k, len(X)): the squared distance of R x + t to y"""
    with np.errstate(all="ignore"):
        d = [(((R[:, r, 0, None] * X[None, :, 0] + R[:, r, 1, None] * X[None, :, 1]) + R[:, r, 2, None] * X[None, :, 2]) + t[:, r, None])
             - Y[None, :, r] for r in range(3)]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def scores(X, Y, R, t, valid, threshold):
    """the exact inlier counts among the live pairs, -1 for an invalid hypothesis"""
    thr = np.float64(np.float32(threshold))
    out = np.full(len(t), -1, np.int64)
    at = np.flatnonzero(valid)
    for lo in range(0, len(at), SLICE):
        s = at[lo:lo + SLICE]
        with np.errstate(invalid="ignore"):
            out[s] = (misses(X, Y, R[s], t[s]) <= thr * thr).sum(axis=1)
    return out


def confident(b, live, T, confidence):
    """the stop rule (1 - w^3)^T <= 1 - confidence: plane_reference's, for samples of three"""
    return plane_confident(b, live, T, 3, confidence)


def align(source, target, src_index, tgt_index, threshold, similarity=0.9, max_trials=100000, confidence=0.999, seed=0):
    """-> (result dict, inliers uint8 (m,))"""
    S32 = np.asarray(source, np.float32).reshape(-1, 3)
    T32 = np.asarray(target, np.float32).reshape(-1, 3)
    si, ti = np.asarray(src_index, np.int64).reshape(-1), np.asarray(tgt_index, np.int64).reshape(-1)
    if len(si) != len(ti):
        raise Invalid("indices")
    m = len(si)
    check(len(S32), len(T32), m, threshold, similarity, max_trials, confidence)
    flags = np.zeros(m, np.uint8)
    if m == 0:
        return nothing(), flags
    in_range = (si >= 0) & (si < len(S32)) & (ti >= 0) & (ti < len(T32))
    is_live = in_range.copy()
    is_live[in_range] = np.all(np.isfinite(S32[si[in_range]]), axis=1) & np.all(np.isfinite(T32[ti[in_range]]), axis=1)
    pair = np.flatnonzero(is_live)
    live = len(pair)
    if live < 3:
        return nothing(m, live), flags
    X, Y = S32[si[pair]].astype(np.float64), T32[ti[pair]].astype(np.float64)
    best, best_h, T, nvalid = -1, -1, 0, 0
    for first in range(0, max_trials, BATCH):
        h = np.arange(first, min(first + BATCH, max_trials))
        R, t, valid = hypotheses(X, Y, seed, h, similarity)
        sc = scores(X, Y, R, t, valid, threshold)
        nvalid += int(valid.sum())
        at = int(np.argmax(sc))                       # the first of equal maxima: the lowest h
        if sc[at] > best:                             # (a later batch wins only with a higher score)
            best, best_h = int(sc[at]), int(h[at])
        T = int(h[-1]) + 1
        if best > 0 and confidence > 0 and confident(best, live, T, confidence):
            break
    if best < 0:
        return nothing(m, live, T, nvalid), flags
    R, t, _ = hypotheses(X, Y, seed, [best_h], similarity)
    d2 = misses(X, Y, R, t)[0]
    thr = np.float64(np.float32(threshold))
    with np.errstate(invalid="ignore"):
        inl = d2 <= thr * thr
    flags[pair[inl]] = 1
    count = int(inl.sum())
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R[0], t[0]
    out = {"found": 1, "pairs": m, "live": live, "trials": T, "valid": nvalid, "inliers": count, "transform": M,
           "rms": float(np.sqrt(tree_sum(d2[inl]) / np.float64(count))) if count else 0.0}
    return out, flags


# ---- the clouds of the tests ----------------------------------------------------------------------------------------------

BUMPS = np.array([[8, 9, 4, 3], [22, 12, -3, 4], [14, 24, 5, 2.5], [27, 27, 3, 3.5], [6, 25, -2.5, 2], [18, 5, 2, 1.8]], np.float64)


def bumpy_surface(xy):
    """(points (n, 3), unit normals (n, 3)) of the height field z = 10 + the sum of six Gaussian bumps (cx, cy, height, sigma)"""
    x, y = xy[:, 0], xy[:, 1]
    z = np.full(len(xy), 10.0)
    zx, zy = np.zeros(len(xy)), np.zeros(len(xy))
    for cx, cy, height, sigma in BUMPS:
        g = height * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * sigma * sigma))
        z += g
        zx += -g * (x - cx) / (sigma * sigma)
        zy += -g * (y - cy) / (sigma * sigma)
    nrm = np.stack([-zx, -zy, np.ones(len(xy))], axis=1)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return np.stack([x, y, z], axis=1), nrm


def rotation(axis, degrees):
    """Rodrigues' matrix (the tests' truth; not part of the contract)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(degrees)
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def angle_between(Ra, Rb):
    """the angle of Ra Rb^T in degrees"""
    c = (np.trace(Ra @ Rb.T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def planted_scans(n=1500, cut=20.0, degrees=97.0, axis=(1.0, 2.0, 3.0), shift=(5.0, -3.0, 4.0), seed=11):
    """the planted case: a target of n points of the bumpy surface over [1, 31]^2 and an independently drawn source of n
    points cut at x < cut, turned and shifted; the draws come from the project's counter hash
    -> (source, source normals, target, target normals, R0, shift), float32 clouds; source = R0^T (p - shift), so that the
    motion that carries the source back onto the target is (R0, shift)"""
    c = np.arange(n, dtype=np.uint64)
    txy = 1.0 + 30.0 * np.stack([uniform(seed, 4 * c), uniform(seed, 4 * c + np.uint64(1))], axis=1)
    sxy = 1.0 + 30.0 * np.stack([uniform(seed, 4 * c + np.uint64(2)), uniform(seed, 4 * c + np.uint64(3))], axis=1)
    sxy = sxy[sxy[:, 0] < cut]
    tp, tn = bumpy_surface(txy)
    sp, sn = bumpy_surface(sxy)
    R0 = rotation(axis, degrees)
    sp = (sp - np.asarray(shift)) @ R0            # rows: R0^T (p - shift)
    sn = sn @ R0
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return f32(sp), f32(sn), f32(tp), f32(tn), R0, np.asarray(shift, np.float64)


def moved_pairs(seed, m, share, noise=0.01, box=20.0):
    """m matched pairs of which about `share` follow one rigid motion (to within `noise`) and the rest are random
    -> (source (m, 3), target (m, 3), R, t); pair c is (source[c], target[c])"""
    rng = np.random.default_rng(seed)
    R = rotation(rng.normal(size=3), rng.uniform(30.0, 170.0))
    t = rng.uniform(-5.0, 5.0, 3)
    src = rng.uniform(0.0, box, (m, 3))
    tgt = src @ R.T + t + rng.uniform(-noise, noise, (m, 3))
    wrong = rng.uniform(size=m) >= share
    tgt[wrong] = rng.uniform(-box, box, (int(wrong.sum()), 3))
    return np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32), R, t
