"""Numpy restatement of the contract of fi_plane_fit / fi_planes_segment (include/fi_hip.h): the dominant
hyperplanes of a point cloud by RANSAC with an exact inlier count and least-squares refits.  Test infrastructure, independent
of the device code.  Every floating-point step is written the way the contract states it -- fp64 from the fp32 coordinates,
one rounding per operation, every sum in its stated order -- so that the masks, labels and figures returned are the bytes the
device must produce.  Only numpy, meshpts_reference.uniform / tree_sum and normals_reference.jacobi."""
import numpy as np

from meshpts_reference import tree_sum, uniform
from normals_reference import jacobi

BATCH = 1024
SLICE = 128          # hypotheses scored at a time (memory only)


class Invalid(Exception):
    """what the device answers with FI_ERR_INVALID"""


class Unsupported(Exception):
    """what the device answers with FI_ERR_UNSUPPORTED"""


def check(ndim, n, threshold, max_trials, confidence, refine, axis, min_cos):
    thr, mc = np.float32(threshold), np.float32(min_cos)
    if ndim not in (2, 3) or n < 0:
        raise Invalid("ndim, n")
    if not (thr >= 0 and np.isfinite(thr)):
        raise Invalid("threshold")
    if not 1 <= max_trials <= 2 ** 20:
        raise Invalid("max_trials")
    if not 0.0 <= confidence < 1.0:
        raise Invalid("confidence")
    if not 0 <= refine <= 16:
        raise Invalid("refine")
    if not 0 <= mc <= 1:
        raise Invalid("min_cos")
    if mc > 0:
        ax = np.asarray(axis, np.float32)[:ndim]
        if not np.all(np.isfinite(ax)) or not np.any(ax != 0):
            raise Invalid("axis")
    if n >= 2 ** 31:
        raise Unsupported("n")


def nothing(candidates=0, trials=0):
    return {"found": 0, "refits": 0, "inliers": 0, "candidates": candidates, "trials": trials, "normal": np.zeros(3), "offset": 0.0,
            "rms": 0.0}


def hypotheses(P, cand, seed, h, axis=None, min_cos=0.0):
    """(n (k, D), d (k,), valid (k,)) of the hypotheses h (k,) over the candidate list cand of the float64 points P"""
    D, m = P.shape[1], len(cand)
    h = np.asarray(h, np.uint64)
    j = [np.minimum(np.floor(uniform(seed, h * np.uint64(D) + np.uint64(k)) * np.float64(m)).astype(np.int64), m - 1) for k in range(D)]
    a, b = P[cand[j[0]]], P[cand[j[1]]]
    valid = j[0] != j[1]
    with np.errstate(all="ignore"):
        if D == 3:
            c = P[cand[j[2]]]
            valid &= (j[0] != j[2]) & (j[1] != j[2])
            u, w = b - a, c - a
            n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                          u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
        else:
            t = b - a
            n = np.stack([-t[:, 1], t[:, 0]], axis=1)
        l2 = n[:, 0] * n[:, 0]
        for x in range(1, D):
            l2 = l2 + n[:, x] * n[:, x]
        ln = np.sqrt(l2)
        valid &= np.isfinite(ln) & (ln > 0.0)
        n = n / ln[:, None]
        s = n[:, 0] * a[:, 0]
        for x in range(1, D):
            s = s + n[:, x] * a[:, x]
        d = -s
        if np.float32(min_cos) > 0:
            ax = np.asarray(axis, np.float32)[:D].astype(np.float64)
            mc = np.float64(np.float32(min_cos))
            aa = ax[0] * ax[0]
            t = n[:, 0] * ax[0]
            for x in range(1, D):
                aa = aa + ax[x] * ax[x]
                t = t + n[:, x] * ax[x]
            valid &= t * t >= (mc * mc) * aa
    return n, d, valid


def residuals(P, n, d):
    """e (k, len(P)) of the models (n (k, D), d (k,)): ((n_0 x_0 + n_1 x_1) + n_2 x_2) + d"""
    with np.errstate(all="ignore"):
        e = n[:, 0, None] * P[None, :, 0] + n[:, 1, None] * P[None, :, 1]
        if P.shape[1] == 3:
            e = e + n[:, 2, None] * P[None, :, 2]
        return e + d[:, None]


def scores(P, cand, n, d, valid, threshold):
    """the exact inlier counts among the candidates, -1 for an invalid hypothesis"""
    X, thr = P[cand], np.float64(np.float32(threshold))
    out = np.full(len(d), -1, np.int64)
    for lo in range(0, len(d), SLICE):
        e = residuals(X, n[lo:lo + SLICE], d[lo:lo + SLICE])
        with np.errstate(invalid="ignore"):
            out[lo:lo + SLICE] = (np.abs(e) <= thr).sum(axis=1)
    return np.where(valid, out, -1)


def confident(b, m, T, D, confidence):
    """the stop rule: (1 - w^D)^T <= 1 - confidence by binary exponentiation from the low bit; add, multiply, compare only"""
    w = np.float64(b) / np.float64(m)
    p = w * w
    if D == 3:
        p = p * w
    q = np.float64(1.0) - p
    r, base, e = np.float64(1.0), q, int(T)
    while e:
        if e & 1:
            r = r * base
        base = base * base
        e >>= 1
    return bool(r <= np.float64(1.0) - np.float64(confidence))


def inliers_of(P, is_cand, n, d, threshold):
    e = residuals(P, n[None, :], np.array([d]))[0]
    with np.errstate(invalid="ignore"):
        return is_cand & (np.abs(e) <= np.float64(np.float32(threshold))), e


def moments(X):
    """(centroid (D,), A (D, D)) of the members X (count, D): tree sums, the centroid first"""
    D = X.shape[1]
    c = np.array([tree_sum(X[:, a]) / np.float64(len(X)) for a in range(D)])
    E = X - c
    A = np.zeros((D, D))
    for a in range(D):
        for b in range(a, D):
            A[a, b] = A[b, a] = tree_sum(E[:, a] * E[:, b])
    return c, A


def refit(X):
    """(normal, d) of the least-squares hyperplane through the members X, or None where the normal is not finite"""
    D = X.shape[1]
    c, A = moments(X)
    with np.errstate(all="ignore"):
        lam, V = jacobi(A[None])
    col, lmin = 0, lam[0, 0]
    for x in range(1, D):
        if lam[0, x] < lmin:
            col, lmin = x, lam[0, x]
    n = V[0][:, col].copy()
    if not np.all(np.isfinite(n)):
        return None
    s = n[0] * c[0]
    for x in range(1, D):
        s = s + n[x] * c[x]
    return n, -s


def fit(positions, threshold, max_trials=1024, confidence=0.999, refine=2, seed=0, mask=None, axis=None, min_cos=0.0, taken=None):
    """-> (model dict, inliers uint8 (n,)); taken (n,) bool: points an earlier plane took (fi_planes_segment)"""
    P32 = np.asarray(positions, np.float32)
    if P32.ndim != 2:
        raise Invalid("positions")
    n_pts, D = P32.shape
    check(D, n_pts, threshold, max_trials, confidence, refine, axis if axis is not None else np.zeros(3), min_cos)
    flags = np.zeros(n_pts, np.uint8)
    if n_pts == 0:
        return nothing(), flags
    P = P32.astype(np.float64)
    is_cand = np.all(np.isfinite(P32), axis=1)
    if mask is not None:
        is_cand &= np.asarray(mask).astype(np.uint8) != 0
    if taken is not None:
        is_cand &= ~taken
    cand = np.flatnonzero(is_cand)
    m = len(cand)
    if m < D:
        return nothing(m, 0), flags
    best, best_h, T = -1, -1, 0
    for first in range(0, max_trials, BATCH):
        h = np.arange(first, min(first + BATCH, max_trials))
        n, d, valid = hypotheses(P, cand, seed, h, axis, min_cos)
        sc = scores(P, cand, n, d, valid, threshold)
        at = int(np.argmax(sc))                       # the first of equal maxima: the lowest h
        if sc[at] > best:                             # (a later batch wins only with a higher score)
            best, best_h = int(sc[at]), int(h[at])
        T = int(h[-1]) + 1
        if best > 0 and confidence > 0 and confident(best, m, T, D, confidence):
            break
    if best < 0:
        return nothing(m, T), flags
    n, d, _ = hypotheses(P, cand, seed, [best_h], axis, min_cos)
    n, d = n[0], d[0]
    inl, e = inliers_of(P, is_cand, n, d, threshold)
    refits = 0
    for _ in range(refine):
        members = np.flatnonzero(inl)
        if len(members) < D:
            break
        got = refit(P[members])
        if got is None:
            break
        n, d = got
        refits += 1
        inl, e = inliers_of(P, is_cand, n, d, threshold)
    big = n[0]
    for x in range(1, D):
        if abs(n[x]) > abs(big):
            big = n[x]
    if big < 0.0:
        n, d = -n, -d
    count = int(inl.sum())
    ee = e[inl]
    normal = np.zeros(3)
    normal[:D] = n
    model = {"found": 1, "refits": refits, "inliers": count, "candidates": m, "trials": T, "normal": normal, "offset": float(d),
             "rms": float(np.sqrt(tree_sum(ee * ee) / np.float64(count))) if count else 0.0}
    return model, inl.astype(np.uint8)


def segment(positions, threshold, max_planes, min_inliers=0, max_trials=1024, confidence=0.999, refine=2, seed=0, mask=None, axis=None,
            min_cos=0.0):
    """-> (labels int32 (n,), list of model dicts)"""
    P32 = np.asarray(positions, np.float32)
    if P32.ndim != 2:
        raise Invalid("positions")
    check(P32.shape[1], len(P32), threshold, max_trials, confidence, refine, axis if axis is not None else np.zeros(3), min_cos)
    if max_planes < 1 or min_inliers < 0:
        raise Invalid("max_planes, min_inliers")
    labels = np.full(len(P32), -1, np.int32)
    models = []
    for p in range(max_planes):
        model, inl = fit(P32, threshold, max_trials, confidence, refine, (int(seed) + p) & (2 ** 64 - 1), mask, axis, min_cos, labels >= 0)
        if not model["found"] or model["inliers"] < min_inliers:
            break
        labels[inl != 0] = p
        models.append(model)
    return labels, models


def planted_cloud(seed=4, n=1500, floor=2000):
    """the sphere scan of the tests (util.sphere_points in a 32^3 lattice, radius 9.3, noise 0.05) standing on a floor: `floor`
    points on the tangent plane z = 6.2 with x, y in [0, 31] and z noise +-0.05, shuffled -> (positions, is_floor)"""
    from util import sphere_points
    rng = np.random.default_rng(seed)
    pos, _ = sphere_points(rng, [32, 32, 32], n, noise=0.05)
    ground = np.stack([rng.uniform(0.0, 31.0, floor), rng.uniform(0.0, 31.0, floor), 6.2 + rng.uniform(-0.05, 0.05, floor)], axis=1)
    allp = np.concatenate([pos, ground.astype(np.float32)])
    flag = np.concatenate([np.zeros(n, bool), np.ones(floor, bool)])
    perm = rng.permutation(len(allp))
    return np.ascontiguousarray(allp[perm], np.float32), flag[perm]


def plane_cloud(seed, n, share, ndim=3, threshold=0.1, box=32.0):
    """n points in a box of side `box`: about `share` of them within `threshold` / 2 of a tilted hyperplane through the
    middle, the rest uniform -> positions float32 (n, ndim)"""
    rng = np.random.default_rng(seed)
    normal = rng.normal(size=ndim)
    normal /= np.linalg.norm(normal)
    k = int(round(share * n))
    x = rng.uniform(0.0, box, (n, ndim))
    on = x[:k] - box / 2
    on -= np.outer(on @ normal, normal)
    x[:k] = on + box / 2 + np.outer(rng.uniform(-0.5, 0.5, k) * threshold, normal)
    return np.ascontiguousarray(x[rng.permutation(n)], np.float32)
