"""Numpy restatement of the contract of fi_shape_fit / fi_shapes_segment (include/fi_hip.h): spheres (circles
in 2-D) and cylinders of a point cloud by RANSAC with an exact inlier count and algebraic least-squares refits.  Test
infrastructure, independent of the device code.  Every floating-point step is written the way the contract states it -- fp64
from the fp32 inputs, one rounding per operation, every sum in its stated order -- so that the masks, labels and figures
returned are the bytes the device must produce.  Only numpy, meshpts_reference.uniform / tree_sum and
normals_reference.jacobi."""
import numpy as np

from meshpts_reference import tree_sum, uniform
from normals_reference import jacobi

BATCH = 1024
SLICE = 64           # hypotheses scored at a time (memory only)
SPHERE, CYLINDER = 0, 1


class Invalid(Exception):
    """what the device answers with FI_ERR_INVALID"""


class Unsupported(Exception):
    """what the device answers with FI_ERR_UNSUPPORTED"""


def sample_size(kind, ndim):
    """S: the points a hypothesis draws"""
    return 2 if kind == CYLINDER else ndim + 1


def check(kind, ndim, n, has_normals, threshold, r_min, r_max, normal_cos, max_trials, confidence, refine):
    thr, lo, hi, mc = np.float32(threshold), np.float32(r_min), np.float32(r_max), np.float32(normal_cos)
    if ndim not in (2, 3) or n < 0:
        raise Invalid("ndim, n")
    if kind not in (SPHERE, CYLINDER):
        raise Invalid("kind")
    if kind == CYLINDER and ndim == 2:
        raise Unsupported("a cylinder in 2-D")
    if kind == CYLINDER and not has_normals:
        raise Invalid("a cylinder without normals")
    if not (thr >= 0 and np.isfinite(thr)):
        raise Invalid("threshold")
    if not lo >= 0 or not hi >= lo:                          # (a NaN fails both)
        raise Invalid("r_min, r_max")
    if not 0 <= mc <= 1 or (mc > 0 and not has_normals):
        raise Invalid("normal_cos")
    if not 1 <= max_trials <= 2 ** 20:
        raise Invalid("max_trials")
    if not 0.0 <= confidence < 1.0:
        raise Invalid("confidence")
    if not 0 <= refine <= 16:
        raise Invalid("refine")
    if n >= 2 ** 31:
        raise Unsupported("n")


def nothing(candidates=0, trials=0):
    return {"found": 0, "kind": 0, "refits": 0, "inliers": 0, "candidates": candidates, "trials": trials, "center": np.zeros(3),
            "axis": np.zeros(3), "radius": 0.0, "extent": np.zeros(2), "rms": 0.0}


def dot(a, b):
    """the products summed over ascending axes (the last axis of the arrays)"""
    s = a[..., 0] * b[..., 0]
    for x in range(1, a.shape[-1]):
        s = s + a[..., x] * b[..., x]
    return s


def unit_normals(normals):
    """(unit normals float64, usable) of the fp32 normals: the length is the square root of the squares summed over ascending
    axes; usable where every component is finite and the length is finite and > 0"""
    N32 = np.asarray(normals, np.float32)
    N = N32.astype(np.float64)
    with np.errstate(all="ignore"):
        ln = np.sqrt(dot(N, N))
        ok = np.all(np.isfinite(N32), axis=1) & np.isfinite(ln) & (ln > 0.0)
        return N / ln[:, None], ok


def cramer(M, r):
    """(x (k, D), ok (k,)) of M x = r for M (k, D, D), r (k, D): cofactors and determinant in the contract's order; ok is false
    where the determinant is not finite or is 0"""
    D = M.shape[-1]
    with np.errstate(all="ignore"):
        if D == 2:
            det = M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]
            x = np.stack([(M[:, 1, 1] * r[:, 0] - M[:, 0, 1] * r[:, 1]) / det, (M[:, 0, 0] * r[:, 1] - M[:, 1, 0] * r[:, 0]) / det], axis=1)
        else:
            C = np.empty_like(M)
            for i in range(3):
                for j in range(3):
                    i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
                    C[:, i, j] = M[:, i1, j1] * M[:, i2, j2] - M[:, i1, j2] * M[:, i2, j1]
            det = (M[:, 0, 0] * C[:, 0, 0] + M[:, 0, 1] * C[:, 0, 1]) + M[:, 0, 2] * C[:, 0, 2]
            x = np.stack([((C[:, 0, j] * r[:, 0] + C[:, 1, j] * r[:, 1]) + C[:, 2, j] * r[:, 2]) / det for j in range(3)], axis=1)
        return x, np.isfinite(det) & (det != 0.0)


def draws(seed, h, S, m):
    """(j (S, k), distinct (k,)): the list positions hypothesis h draws among m candidates"""
    h = np.asarray(h, np.uint64)
    j = [np.minimum(np.floor(uniform(seed, h * np.uint64(S) + np.uint64(k)) * np.float64(m)).astype(np.int64), m - 1) for k in range(S)]
    distinct = np.ones(len(h), bool)
    for k in range(S):
        for q in range(k):
            distinct &= j[q] != j[k]
    return j, distinct


def hypotheses(kind, P, U, cand, seed, h, r_min=0.0, r_max=np.inf):
    """(c (k, D) the centre or the axis point, a (k, 3) the axis (zeros for a sphere), r (k,), valid (k,)) of the hypotheses
    h (k,) over the candidate list cand of the float64 points P and unit normals U"""
    D, m = P.shape[1], len(cand)
    S = sample_size(kind, D)
    j, valid = draws(seed, h, S, m)
    p = [P[cand[j[k]]] for k in range(S)]
    with np.errstate(all="ignore"):
        if kind == SPHERE:
            q = np.stack([p[k] - p[0] for k in range(1, S)], axis=1)            # (k, D, D): the rows q_1 .. q_D
            half = np.stack([0.5 * dot(q[:, k], q[:, k]) for k in range(D)], axis=1)
            cp, ok = cramer(q, half)
            valid &= ok
            c = p[0] + cp
            r = np.sqrt(dot(cp, cp))
            a = np.zeros((len(c), 3))
        else:
            n0, n1 = U[cand[j[0]]], U[cand[j[1]]]
            a = np.stack([n0[:, 1] * n1[:, 2] - n0[:, 2] * n1[:, 1], n0[:, 2] * n1[:, 0] - n0[:, 0] * n1[:, 2],
                          n0[:, 0] * n1[:, 1] - n0[:, 1] * n1[:, 0]], axis=1)
            ln = np.sqrt(dot(a, a))
            valid &= np.isfinite(ln) & (ln > 0.0)
            a = a / ln[:, None]
            d = p[1] - p[0]
            g00, g01, g11, b0, b1 = dot(n0, n0), dot(n0, n1), dot(n1, n1), dot(n0, d), dot(n1, d)
            det = g00 * g11 - g01 * g01
            valid &= np.isfinite(det) & (det != 0.0)
            s = (b0 * g11 - g01 * b1) / det
            c = p[0] + s[:, None] * n0
            r = np.abs(s)
        lo, hi = np.float64(np.float32(r_min)), np.float64(np.float32(r_max))
        valid &= np.isfinite(r) & (lo <= r) & (r <= hi)
    return c, a, r, valid


def band(r, threshold):
    """(lo2, hi2): the squared radii a point's squared distance lies between, both inclusive"""
    thr = np.float64(np.float32(threshold))
    lo = np.maximum(r - thr, 0.0)
    hi = r + thr
    return lo * lo, hi * hi


def offsets(kind, X, c, a):
    """(g (k, len(X), D), s (k, len(X))): the vector from the model to each point -- x - c for a sphere; for a cylinder v = x - q,
    t = v . a, g = v - t a -- and its squares summed over ascending axes"""
    with np.errstate(all="ignore"):
        g = X[None, :, :] - c[:, None, :]
        if kind == CYLINDER:
            t = dot(g, a[:, None, :])
            g = g - t[:, :, None] * a[:, None, :]
        return g, dot(g, g)


def inside(kind, X, UX, c, a, r, threshold, normal_cos):
    """(in (k, len(X)) bool, s (k, len(X))) for the models (c, a, r): lo2 <= s <= hi2 and, with normal_cos > 0,
    (n . g)^2 >= (mc mc)(g . g) with g . g > 0"""
    lo2, hi2 = band(r, threshold)
    g, s = offsets(kind, X, c, a)
    with np.errstate(all="ignore"):
        ok = (lo2[:, None] <= s) & (s <= hi2[:, None])
        mc = np.float64(np.float32(normal_cos))
        if mc > 0:
            nd = dot(UX[None, :, :], g)
            ok &= (s > 0.0) & (nd * nd >= (mc * mc) * s)
    return ok, s


def scores(kind, P, U, cand, c, a, r, valid, threshold, normal_cos):
    """the exact inlier counts among the candidates, -1 for an invalid hypothesis"""
    X, UX = P[cand], (U[cand] if U is not None else None)
    out = np.full(len(r), -1, np.int64)
    for lo in range(0, len(r), SLICE):
        ok, _ = inside(kind, X, UX, c[lo:lo + SLICE], a[lo:lo + SLICE], r[lo:lo + SLICE], threshold, normal_cos)
        out[lo:lo + SLICE] = ok.sum(axis=1)
    return np.where(valid, out, -1)


def confident(b, m, T, S, confidence):
    """the stop rule: (1 - w^S)^T <= 1 - confidence by binary exponentiation from the low bit; add, multiply, compare only"""
    w = np.float64(b) / np.float64(m)
    p = w
    for _ in range(1, S):
        p = p * w
    q = np.float64(1.0) - p
    r, base, e = np.float64(1.0), q, int(T)
    while e:
        if e & 1:
            r = r * base
        base = base * base
        e >>= 1
    return bool(r <= np.float64(1.0) - np.float64(confidence))


def inliers_of(kind, P, U, is_cand, c, a, r, threshold, normal_cos):
    ok, s = inside(kind, P, U, c[None], a[None], np.array([r]), threshold, normal_cos)
    return is_cand & ok[0], s[0]


def kasa(Y):
    """(c' (D,), r, ok) of the algebraic circle / sphere through the centred members Y (count, D): one pass of sums, then
    (sum y y^T) c' = 1/2 sum y w, r = sqrt(c' . c' + sum w / count)"""
    D, count = Y.shape[1], np.float64(len(Y))
    w = dot(Y, Y)
    M = np.zeros((D, D))
    for a in range(D):
        for b in range(a, D):
            M[a, b] = M[b, a] = tree_sum(Y[:, a] * Y[:, b])
    rhs = np.array([0.5 * tree_sum(Y[:, a] * w) for a in range(D)])
    sw = tree_sum(w)
    cp, ok = cramer(M[None], rhs[None])
    cp = cp[0]
    with np.errstate(all="ignore"):
        r = np.sqrt(dot(cp, cp) + sw / count)
    return cp, r, bool(ok[0])


def centroid(X):
    return np.array([tree_sum(X[:, a]) / np.float64(len(X)) for a in range(X.shape[1])])


def refit(kind, X, UX):
    """(c, a, r) of the least-squares model through the members X (unit normals UX), or None where the solve fails or
    anything is not finite"""
    m = centroid(X)
    if kind == SPHERE:
        cp, r, ok = kasa(X - m)
        c, a = m + cp, np.zeros(3)
    else:
        N = np.zeros((3, 3))
        for p in range(3):
            for q in range(p, 3):
                N[p, q] = N[q, p] = tree_sum(UX[:, p] * UX[:, q])
        with np.errstate(all="ignore"):
            lam, V = jacobi(N[None])
        col, lmin = 0, lam[0, 0]
        for x in range(1, 3):
            if lam[0, x] < lmin:
                col, lmin = x, lam[0, x]
        a = V[0][:, col].copy()
        e1, e2 = [V[0][:, x].copy() for x in range(3) if x != col]
        if not (np.all(np.isfinite(a)) and np.all(np.isfinite(e1)) and np.all(np.isfinite(e2))):
            return None
        Y = X - m
        cp, r, ok = kasa(np.stack([dot(Y, e1[None]), dot(Y, e2[None])], axis=1))
        c = (m + cp[0] * e1) + cp[1] * e2
    if not ok or not np.all(np.isfinite(c)) or not np.isfinite(r):
        return None
    return c, a, r


def fit(positions, kind, threshold, r_min=0.0, r_max=np.inf, normals=None, normal_cos=0.0, max_trials=1024, confidence=0.999, refine=2,
        seed=0, mask=None, taken=None):
    """-> (model dict, inliers uint8 (n,)); taken (n,) bool: points an earlier shape took (fi_shapes_segment)"""
    P32 = np.asarray(positions, np.float32)
    if P32.ndim != 2:
        raise Invalid("positions")
    n_pts, D = P32.shape
    check(kind, D, n_pts, normals is not None, threshold, r_min, r_max, normal_cos, max_trials, confidence, refine)
    flags = np.zeros(n_pts, np.uint8)
    if n_pts == 0:
        return nothing(), flags
    S = sample_size(kind, D)
    P = P32.astype(np.float64)
    is_cand = np.all(np.isfinite(P32), axis=1)
    U = None
    if normals is not None:
        U, usable = unit_normals(normals)
        is_cand &= usable
    if mask is not None:
        is_cand &= np.asarray(mask).astype(np.uint8) != 0
    if taken is not None:
        is_cand &= ~taken
    cand = np.flatnonzero(is_cand)
    m = len(cand)
    if m < S:
        return nothing(m, 0), flags
    lo, hi = np.float64(np.float32(r_min)), np.float64(np.float32(r_max))
    best, best_h, T = -1, -1, 0
    for first in range(0, max_trials, BATCH):
        h = np.arange(first, min(first + BATCH, max_trials))
        c, a, r, valid = hypotheses(kind, P, U, cand, seed, h, r_min, r_max)
        sc = scores(kind, P, U, cand, c, a, r, valid, threshold, normal_cos)
        at = int(np.argmax(sc))                       # the first of equal maxima: the lowest h
        if sc[at] > best:                             # (a later batch wins only with a higher score)
            best, best_h = int(sc[at]), int(h[at])
        T = int(h[-1]) + 1
        if best > 0 and confidence > 0 and confident(best, m, T, S, confidence):
            break
    if best < 0:
        return nothing(m, T), flags
    c, a, r, _ = hypotheses(kind, P, U, cand, seed, [best_h], r_min, r_max)
    c, a, r = c[0], a[0], r[0]
    inl, s = inliers_of(kind, P, U, is_cand, c, a, r, threshold, normal_cos)
    refits = 0
    for _ in range(refine):
        members = np.flatnonzero(inl)
        if len(members) < S + 1:
            break
        got = refit(kind, P[members], U[members] if U is not None else None)
        if got is None or not lo <= got[2] <= hi:
            break
        c, a, r = got
        refits += 1
        inl, s = inliers_of(kind, P, U, is_cand, c, a, r, threshold, normal_cos)
    count = int(inl.sum())
    center, axis, extent = np.zeros(3), np.zeros(3), np.zeros(2)
    center[:D] = c
    if kind == CYLINDER:
        big = a[0]
        for x in range(1, 3):
            if abs(a[x]) > abs(big):
                big = a[x]
        axis[:] = -a if big < 0.0 else a
        if count:
            t = dot(P[inl] - c[None], axis[None])
            extent[:] = [t.min(), t.max()]
    e = np.sqrt(s[inl]) - r
    model = {"found": 1, "kind": kind, "refits": refits, "inliers": count, "candidates": m, "trials": T, "center": center, "axis": axis,
             "radius": float(r), "extent": extent, "rms": float(np.sqrt(tree_sum(e * e) / np.float64(count))) if count else 0.0}
    return model, inl.astype(np.uint8)


def segment(positions, kind, threshold, max_shapes, min_inliers=0, r_min=0.0, r_max=np.inf, normals=None, normal_cos=0.0, max_trials=1024,
            confidence=0.999, refine=2, seed=0, mask=None):
    """-> (labels int32 (n,), list of model dicts)"""
    P32 = np.asarray(positions, np.float32)
    if P32.ndim != 2:
        raise Invalid("positions")
    check(kind, P32.shape[1], len(P32), normals is not None, threshold, r_min, r_max, normal_cos, max_trials, confidence, refine)
    if max_shapes < 1 or min_inliers < 0:
        raise Invalid("max_shapes, min_inliers")
    labels = np.full(len(P32), -1, np.int32)
    models = []
    for p in range(max_shapes):
        model, inl = fit(P32, kind, threshold, r_min, r_max, normals, normal_cos, max_trials, confidence, refine,
                         (int(seed) + p) & (2 ** 64 - 1), mask, labels >= 0)
        if not model["found"] or model["inliers"] < min_inliers:
            break
        labels[inl != 0] = p
        models.append(model)
    return labels, models


# ---- the clouds of the tests ----------------------------------------------------------------------------------------------

def _frame(axis):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    e1 = np.cross(a, [1.0, 0.0, 0.0] if abs(a[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    return a, e1, np.cross(a, e1)


def sphere_part(rng, n, center, radius, noise, ndim=3):
    """(positions, outward normals) of n points on the sphere (circle), moved radially by uniform +-noise"""
    d = rng.normal(size=(n, ndim))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.asarray(center, np.float64)[:ndim] + d * (radius + rng.uniform(-noise, noise, n))[:, None], d


def cylinder_part(rng, n, point, axis, radius, length, noise, normal_noise=0.0):
    """(positions, normals) of n points on the cylinder about the line through `point` along `axis`, t in +-length / 2"""
    a, e1, e2 = _frame(axis)
    phi, t = rng.uniform(0.0, 2.0 * np.pi, n), rng.uniform(-length / 2, length / 2, n)
    d = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    nrm = d + rng.normal(size=(n, 3)) * normal_noise
    return np.asarray(point, np.float64) + t[:, None] * a + d * (radius + rng.uniform(-noise, noise, n))[:, None], nrm


def shape_cloud(seed, n, share, kind, ndim=3, threshold=0.05, box=8.0):
    """n points in a box of side `box`: about `share` of them within `threshold` / 2 of a sphere (circle) of radius 2 or a
    cylinder of radius 1 in the middle, the rest uniform; every point carries a normal (the shape's own, slightly perturbed, or
    a random one) -> (positions float32 (n, ndim), normals float32 (n, ndim))"""
    rng = np.random.default_rng(seed)
    k = int(round(share * n))
    x, nr = rng.uniform(0.0, box, (n, ndim)), rng.normal(size=(n, ndim))
    mid = np.full(ndim, box / 2)
    if kind == SPHERE:
        x[:k], nr[:k] = sphere_part(rng, k, mid, 2.0, threshold / 2, ndim)
        nr[:k] += rng.normal(size=(k, ndim)) * 0.02
    else:
        x[:k], nr[:k] = cylinder_part(rng, k, mid, rng.normal(size=3), 1.0, 5.0, threshold / 2, 0.02)
    perm = rng.permutation(n)
    return np.ascontiguousarray(x[perm], np.float32), np.ascontiguousarray(nr[perm], np.float32)


def _floor_and_strays(rng, floor, strays):
    ground = np.stack([rng.uniform(-4.0, 6.0, floor), rng.uniform(-3.0, 7.0, floor), np.zeros(floor)], axis=1)
    up = np.tile([0.0, 0.0, 1.0], (floor, 1))
    return (np.concatenate([ground, rng.uniform(-4.0, 7.0, (strays, 3))]), np.concatenate([up, rng.normal(size=(strays, 3))]))


def planted_sphere(seed=1, n=1500, floor=2000, strays=100):
    """scene (a): a sphere of radius 2 at (1, 2, 2), noise 0.01, resting on the plane z = 0, and stray points, shuffled
    -> (positions, normals, planted (n,) bool)"""
    rng = np.random.default_rng(seed)
    x, nr = sphere_part(rng, n, [1.0, 2.0, 2.0], 2.0, 0.01)
    ox, on = _floor_and_strays(rng, floor, strays)
    perm = rng.permutation(n + floor + strays)
    flag = np.concatenate([np.ones(n, bool), np.zeros(floor + strays, bool)])
    return (np.ascontiguousarray(np.concatenate([x, ox])[perm], np.float32), np.ascontiguousarray(np.concatenate([nr, on])[perm], np.float32),
            flag[perm])


CYL_POINT, CYL_AXIS = np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0, 2.0]) / 3.0


def planted_cylinder(seed=1, n=1500, floor=2000, strays=100):
    """scene (b): a cylinder of radius 0.5 and length 6 about the line through (1, 2, 3) along (1, 2, 2) / 3, noise 0.01, its
    normals perturbed by 0.05, with scene (a)'s plane and strays -> (positions, normals, planted (n,) bool)"""
    rng = np.random.default_rng(seed)
    x, nr = cylinder_part(rng, n, CYL_POINT, CYL_AXIS, 0.5, 6.0, 0.01, 0.05)
    ox, on = _floor_and_strays(rng, floor, strays)
    perm = rng.permutation(n + floor + strays)
    flag = np.concatenate([np.ones(n, bool), np.zeros(floor + strays, bool)])
    return (np.ascontiguousarray(np.concatenate([x, ox])[perm], np.float32), np.ascontiguousarray(np.concatenate([nr, on])[perm], np.float32),
            flag[perm])
