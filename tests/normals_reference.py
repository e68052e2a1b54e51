"""Numpy oracle of the k-nearest-point and normal-estimation contracts (include/fi_hip.h fi_knn, fi_estimate_normals;
DESIGN.md 4.11).  knn: a brute force over every (query, point) pair in chunks with nearest_reference.sq_dist's fp32
arithmetic and a stable argsort, so that equal s go to the smallest index.  estimate_normals: the definition of the local
PCA -- fp64, one rounding per operation, only + - * / sqrt, every sum from 0.0 in the stated order, a cyclic Jacobi iteration
of a fixed number of sweeps -- written for all points at once (elementwise numpy operations round like the scalar ones).
Only numpy."""
import numpy as np

import nearest_reference as R

SWEEPS = 6
MAX_K = 32


def knn(points, queries, ndim, k, max_distance=np.inf, chunk_pairs=1 << 22):
    """(distances float32 (m, k), indices int64 (m, k)): the first k of the pairs (s, j) over the finite points in
    lexicographic order with sqrtf(s) <= max_distance; missing entries +inf / -1 at the end; a non-finite query NaN / -1"""
    if not 1 <= k <= MAX_K:
        raise ValueError("k must be 1..%d" % MAX_K)
    P = R._as_points(points, ndim)
    Q = R._as_points(queries, ndim)
    md = np.float32(max_distance)
    keep = np.flatnonzero(np.all(np.isfinite(P), axis=1))     # ascending: a stable sort keeps the smallest index first
    Pf = P[keep]
    m = Q.shape[0]
    dist = np.full((m, k), np.inf, np.float32)
    idx = np.full((m, k), -1, np.int64)
    qok = np.all(np.isfinite(Q), axis=1)
    dist[~qok] = np.nan
    have = min(k, Pf.shape[0])
    if have > 0:
        rows = np.flatnonzero(qok)
        step = max(1, chunk_pairs // Pf.shape[0])
        with np.errstate(over="ignore"):
            for b in range(0, rows.size, step):
                r = rows[b: b + step]
                s = R.sq_dist(Pf, Q[r])
                order = np.argsort(s, axis=1, kind="stable")[:, :have]
                d = np.sqrt(np.take_along_axis(s, order, axis=1)).astype(np.float32)
                far = d > md
                dist[r, :have] = np.where(far, np.float32(np.inf), d)
                idx[r, :have] = np.where(far, -1, keep[order])
    return dist, idx


def _rotate(A, V, p, q, D):
    """one Jacobi rotation of the pair (p, q) on the symmetric matrices A (n, D, D; both triangles kept equal) and the
    vector matrices V (n, D, D; columns are vectors), skipped where a_pq == 0.  The order of operations:
        theta = (a_qq - a_pp) / (2 a_pq);  t = sign(theta) / (|theta| + sqrt(theta theta + 1));  c = 1 / sqrt(t t + 1);  s = t c
        a_pp <- a_pp - t a_pq;  a_qq <- a_qq + t a_pq;  a_pq <- 0
        the third axis r (3-D):  a_rp <- c a_rp - s a_rq;  a_rq <- s a_rp + c a_rq      (both from the old a_rp, a_rq)
        every row r of V:        v_rp <- c v_rp - s v_rq;  v_rq <- s v_rp + c v_rq      (both from the old v_rp, v_rq)"""
    apq = A[:, p, q]
    on = apq != 0.0
    with np.errstate(all="ignore"):
        theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
        t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        tap = t * apq
        app = A[:, p, p] - tap
        aqq = A[:, q, q] + tap
        A[:, p, p] = np.where(on, app, A[:, p, p])
        A[:, q, q] = np.where(on, aqq, A[:, q, q])
        A[:, p, q] = A[:, q, p] = np.where(on, 0.0, apq)
        for r in range(D):
            if r == p or r == q:
                continue
            arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
            A[:, r, p] = A[:, p, r] = np.where(on, c * arp - s * arq, arp)
            A[:, r, q] = A[:, q, r] = np.where(on, s * arp + c * arq, arq)
        for r in range(D):
            vrp, vrq = V[:, r, p].copy(), V[:, r, q].copy()
            V[:, r, p] = np.where(on, c * vrp - s * vrq, vrp)
            V[:, r, q] = np.where(on, s * vrp + c * vrq, vrq)


def jacobi(A, sweeps=SWEEPS):
    """(diagonal (n, D), vectors (n, D, D)) of the symmetric fp64 matrices A (n, D, D) after `sweeps` cyclic sweeps over
    the pairs (0,1), (0,2), (1,2) -- in 2-D the single pair (0,1); no early exit"""
    A = np.array(A, np.float64)
    n, D, _ = A.shape
    V = np.zeros((n, D, D), np.float64)
    for d in range(D):
        V[:, d, d] = 1.0
    pairs = [(0, 1)] if D == 2 else [(0, 1), (0, 2), (1, 2)]
    for _ in range(sweeps):
        for p, q in pairs:
            _rotate(A, V, p, q, D)
    return np.stack([A[:, d, d] for d in range(D)], axis=1), V


def covariances(points, ndim, idx):
    """(centroids (n, D), covariance sums (n, D, D), m (n,)) of the neighbour lists idx (n, k; -1 at the end): the centroid
    is the sum of the neighbours' coordinates (widened from fp32) from 0.0 in neighbour order divided by m; each covariance
    entry is the sum from 0.0 in neighbour order of (p_a - c_a)(p_b - c_b) -- not divided by m"""
    P = R._as_points(points, ndim).astype(np.float64)
    n, k = idx.shape
    D = ndim
    valid = idx >= 0
    m = valid.sum(axis=1)
    nb = P[np.where(valid, idx, 0)]                           # (n, k, D)
    with np.errstate(all="ignore"):
        c = np.zeros((n, D), np.float64)
        for r in range(k):
            c = np.where(valid[:, r, None], c + nb[:, r, :], c)
        c = c / np.maximum(m, 1)[:, None].astype(np.float64)
        A = np.zeros((n, D, D), np.float64)
        for r in range(k):
            e = nb[:, r, :] - c
            for a in range(D):
                for b in range(a, D):
                    A[:, a, b] = np.where(valid[:, r], A[:, a, b] + e[:, a] * e[:, b], A[:, a, b])
        for a in range(D):
            for b in range(a):
                A[:, a, b] = A[:, b, a]
    return c, A, m


def normals_of(A):
    """(canonical normals (n, D), variation (n,)) of the covariance sums A: the Jacobi column whose diagonal entry is
    smallest (the lowest column on a tie), its component of largest magnitude (the first such axis) made positive;
    variation = that diagonal entry / (the diagonal summed in axis order), 0 where that sum is 0"""
    lam, V = jacobi(A)
    n, D = lam.shape
    col = np.argmin(lam, axis=1)
    nrm = np.take_along_axis(V, col[:, None, None].repeat(D, 1), axis=2)[:, :, 0]
    big = np.argmax(np.abs(nrm), axis=1)
    neg = np.take_along_axis(nrm, big[:, None], axis=1)[:, 0] < 0.0
    nrm = np.where(neg[:, None], -nrm, nrm)
    tot = np.zeros(n, np.float64)
    for d in range(D):
        tot = tot + lam[:, d]
    lmin = np.take_along_axis(lam, col[:, None], axis=1)[:, 0]
    with np.errstate(all="ignore"):
        var = np.where(tot == 0.0, 0.0, lmin / tot)
    return nrm, var


def orient(nrm, towards):
    """flip where w = sum over ascending axes from 0.0 of n_a * towards_a is finite and < 0"""
    w = np.zeros(nrm.shape[0], np.float64)
    with np.errstate(all="ignore"):
        for a in range(nrm.shape[1]):
            w = w + nrm[:, a] * towards[:, a]
    flip = np.isfinite(w) & (w < 0.0)
    return np.where(flip[:, None], -nrm, nrm)


def estimate_normals(points, ndim, k=16, max_distance=np.inf, viewpoints=None, directions=None, neighbours=None):
    """(normals float32 (n, D), variation float32 (n,)) of every point of `points` from its k nearest points, itself
    included.  viewpoints: (1, D) or (n, D), normals turned towards them; directions: (n, D), normals turned along them;
    neither: the canonical sign.  neighbours: the (distances, indices) of knn(points, points, ndim, k, max_distance), if the
    caller has them already."""
    if ndim < 2:
        raise ValueError("normals need 2 or 3 dimensions")
    if k < ndim:
        raise ValueError("k < ndim")
    P = R._as_points(points, ndim)
    n, D = P.shape
    _, idx = neighbours if neighbours is not None else knn(P, P, D, k, max_distance)
    _, A, m = covariances(P, D, idx)
    nrm, var = normals_of(A)
    P64 = P.astype(np.float64)
    with np.errstate(all="ignore"):
        if viewpoints is not None:
            v = R._as_points(viewpoints, D).astype(np.float64)
            if v.shape[0] not in (1, n):
                raise ValueError("viewpoints: one, or one per point")
            nrm = orient(nrm, np.broadcast_to(v, (n, D)) - P64)
        elif directions is not None:
            g = R._as_points(directions, D).astype(np.float64)
            if g.shape[0] != n:
                raise ValueError("directions: one per point")
            nrm = orient(nrm, g)
    bad = ~np.all(np.isfinite(P), axis=1) | (m < D)
    nrm = np.where(bad[:, None], 0.0, nrm).astype(np.float32)
    var = np.where(bad, np.nan, var).astype(np.float32)
    return nrm, var
