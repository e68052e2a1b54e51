"""Numpy definition of the moving-least-squares projection (include/fi_hip.h fi_mls_project): fp64, one
rounding per operation, only + - * / sqrt, every sum from 0.0 in neighbour order, written for all queries at once
(elementwise numpy operations round like the scalar ones).  The neighbours are normals_reference.knn's, the Jacobi iteration
is normals_reference.jacobi -- imported, not copied.  Only numpy."""
import numpy as np

import nearest_reference as NR
import normals_reference as R

MAX_K = 32
PIVOT = 1.0e-15         # kMlsPivot (fi_mls.hip): a Cholesky pivot must exceed PIVOT * W (DESIGN.md 4.25 has the measurements)


def _basis(D, u, v):
    """the quadric's basis over the local coordinates: (1, u, v, uu, uv, vv) in 3-D, (1, u, uu) in 2-D"""
    one = np.ones_like(u)
    return [one, u, v, u * u, u * v, v * v] if D == 3 else [one, u, u * u]


def _dot(a, b):
    """the sum from 0.0 in ascending axes of a_d b_d, over the last axis"""
    s = np.zeros(a.shape[:-1], np.float64)
    for d in range(a.shape[-1]):
        s = s + a[..., d] * b[..., d]
    return s


def frame(lam, V):
    """(normal (n, D), tangents [(n, D)] * (D - 1)) of the Jacobi result: the column of the smallest diagonal entry (the
    lowest on a tie) with its component of largest magnitude (the first such axis) made positive; the remaining columns in
    ascending column order, as they are"""
    n, D = lam.shape
    col = np.argmin(lam, axis=1)
    pick = lambda c: np.take_along_axis(V, c[:, None, None].repeat(D, 1), axis=2)[:, :, 0]  # noqa: E731
    nrm = pick(col)
    big = np.argmax(np.abs(nrm), axis=1)
    neg = np.take_along_axis(nrm, big[:, None], axis=1)[:, 0] < 0.0
    nrm = np.where(neg[:, None], -nrm, nrm)
    tangents = []
    for r in range(D - 1):
        c = np.full(n, r, np.int64)
        c = c + (c >= col)                                   # the r-th column that is not `col`
        tangents.append(pick(c))
    return nrm, tangents


def cholesky_solve(M, rhs, floor):
    """(x (n, NB), ok (n,), pivots (n, NB)) of M x = rhs by an unpivoted Cholesky in a fixed order: column j's pivot is
    m_jj - l_j0 l_j0 - ... - l_j,j-1 l_j,j-1 (subtracted in that order); ok where every pivot is > floor; then
    l_ij = (m_ij - l_i0 l_j0 - ...) / l_jj, y_i = (b_i - l_i0 y_0 - ...) / l_ii, x_i = (y_i - l_i+1,i x_i+1 - ... ) / l_ii
    (ascending rows)."""
    n, NB, _ = M.shape
    L = np.zeros((n, NB, NB), np.float64)
    piv = np.zeros((n, NB), np.float64)
    ok = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for j in range(NB):
            d = M[:, j, j].copy()
            for k in range(j):
                d = d - L[:, j, k] * L[:, j, k]
            piv[:, j] = d
            ok &= d > floor
            L[:, j, j] = np.sqrt(d)
            for i in range(j + 1, NB):
                t = M[:, i, j].copy()
                for k in range(j):
                    t = t - L[:, i, k] * L[:, j, k]
                L[:, i, j] = t / L[:, j, j]
        y = np.zeros((n, NB), np.float64)
        for i in range(NB):
            t = rhs[:, i].copy()
            for k in range(i):
                t = t - L[:, i, k] * y[:, k]
            y[:, i] = t / L[:, i, i]
        x = np.zeros((n, NB), np.float64)
        for i in range(NB - 1, -1, -1):
            t = y[:, i].copy()
            for k in range(i + 1, NB):
                t = t - L[:, k, i] * x[:, k]
            x[:, i] = t / L[:, i, i]
    return x, ok, piv


def project(points, ndim, queries=None, k=32, radius=None, degree=2, max_move=np.inf, guide_normals=None, details=False,
            neighbours=None):
    """(positions float32 (n, D), normals float32 (n, D), curvature float32 (n,), order uint8 (n,)) of the projection of
    `queries` (None: the set's own points) onto the local polynomial surface of `points`.  details=True adds a dict:
    `ratio`, the smallest Cholesky pivot divided by W (those that follow a negative one are NaN and skipped; NaN where the
    quadric was not tried), `m` and `W`.  neighbours: the indices of normals_reference.knn(points, queries, ndim, k' >= k,
    radius), if the caller has them already (a smaller k's list is a prefix of a larger one's)."""
    if ndim not in (2, 3):
        raise ValueError("2 or 3 dimensions")
    if not 1 <= k <= MAX_K:
        raise ValueError("k must be 1..%d" % MAX_K)
    if degree not in (1, 2):
        raise ValueError("degree 1 or 2")
    if not (radius is not None and np.isfinite(radius) and radius > 0):
        raise ValueError("radius > 0 and finite")
    if not max_move >= 0:
        raise ValueError("max_move >= 0")
    D = ndim
    P = NR._as_points(points, D)
    Q = P if queries is None else NR._as_points(queries, D)
    n = Q.shape[0]
    NB = 6 if D == 3 else 3
    h = np.float64(np.float32(radius))
    mm = np.float64(np.float32(max_move))
    idx = neighbours[:, :k] if neighbours is not None else R.knn(P, Q, D, k, np.float32(radius))[1]
    valid = idx >= 0
    m = valid.sum(axis=1)
    safe = np.where(valid, idx, 0)
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    nb = P64[safe]                                           # (n, k, D)
    with np.errstate(all="ignore"):
        # the fp32 s of the list
        s = np.zeros((n, k), np.float32)
        for d in range(D):
            e32 = P[safe][:, :, d] - Q[:, None, d]
            s = s + e32 * e32
        h2 = h * h
        w = 1.0 - s.astype(np.float64) / h2
        w = np.where(w < 0.0, 0.0, w)
        w = (w * w) * w
        w = np.where(valid, w, 0.0)
        positive = (valid & (w > 0.0)).sum(axis=1)
        W = np.zeros(n, np.float64)
        c = np.zeros((n, D), np.float64)
        for r in range(k):
            on = valid[:, r]
            W = np.where(on, W + w[:, r], W)
            c = np.where(on[:, None], c + w[:, r, None] * nb[:, r, :], c)
        c = c / W[:, None]
        A = np.zeros((n, D, D), np.float64)
        for r in range(k):
            e = nb[:, r, :] - c
            for a in range(D):
                we = w[:, r] * e[:, a]
                for b in range(a, D):
                    A[:, a, b] = np.where(valid[:, r], A[:, a, b] + we * e[:, b], A[:, a, b])
        for a in range(D):
            for b in range(a):
                A[:, a, b] = A[:, b, a]
        refused = (m < D) | (positive < D) | ~(W > 0.0) | ~np.all(np.isfinite(Q), axis=1)
        A = np.where(refused[:, None, None], 0.0, A)         # (their Jacobi result is not read)
        lam, V = R.jacobi(A)
        nrm, tan = frame(lam, V)

        # the quadric
        coef = np.zeros((n, NB), np.float64)
        order = np.where(refused, 0, 1).astype(np.uint8)
        ratio = np.full(n, np.nan)
        if degree == 2:
            M = np.zeros((n, NB, NB), np.float64)
            rhs = np.zeros((n, NB), np.float64)
            for r in range(k):
                e = nb[:, r, :] - c
                u = _dot(e, tan[0]) / h
                v = _dot(e, tan[1]) / h if D == 3 else None
                z = _dot(e, nrm) / h
                B = _basis(D, u, v)
                on = valid[:, r]
                for a in range(NB):
                    wb = w[:, r] * B[a]
                    for b in range(a, NB):
                        M[:, a, b] = np.where(on, M[:, a, b] + wb * B[b], M[:, a, b])
                    rhs[:, a] = np.where(on, rhs[:, a] + wb * z, rhs[:, a])
            for a in range(NB):
                for b in range(a):
                    M[:, a, b] = M[:, b, a]
            x, ok, piv = cholesky_solve(M, rhs, PIVOT * W)
            tried = ~refused & (m >= NB)
            quad = tried & ok
            coef = np.where(quad[:, None], x, 0.0)
            order = np.where(quad, 2, order).astype(np.uint8)
            ratio = np.where(tried, np.nanmin(np.where(tried[:, None], piv / W[:, None], 0.0), axis=1), np.nan)

        # the projection of q
        eq = Q64 - c
        u0 = _dot(eq, tan[0]) / h
        if D == 3:
            v0 = _dot(eq, tan[1]) / h
            p = coef[:, 0] + coef[:, 1] * u0
            p = p + coef[:, 2] * v0
            p = p + coef[:, 3] * (u0 * u0)
            p = p + coef[:, 4] * (u0 * v0)
            p = p + coef[:, 5] * (v0 * v0)
            pu = coef[:, 1] + (2.0 * coef[:, 3]) * u0
            pu = pu + coef[:, 4] * v0
            pv = coef[:, 2] + coef[:, 4] * u0
            pv = pv + (2.0 * coef[:, 5]) * v0
            puu, puv, pvv = 2.0 * coef[:, 3], coef[:, 4], 2.0 * coef[:, 5]
            x1 = c + h * ((u0[:, None] * tan[0] + v0[:, None] * tan[1]) + p[:, None] * nrm)
            g = (nrm - pu[:, None] * tan[0]) - pv[:, None] * tan[1]
            a1 = 1.0 + pu * pu
            b1 = 1.0 + pv * pv
            gg = a1 + pv * pv
            num = (b1 * puu - ((2.0 * pu) * pv) * puv) + a1 * pvv
            curv = num / ((2.0 * h) * (gg * np.sqrt(gg)))
        else:
            p = coef[:, 0] + coef[:, 1] * u0
            p = p + coef[:, 2] * (u0 * u0)
            pu = coef[:, 1] + (2.0 * coef[:, 2]) * u0
            puu = 2.0 * coef[:, 2]
            x1 = c + h * (u0[:, None] * tan[0] + p[:, None] * nrm)
            g = nrm - pu[:, None] * tan[0]
            gg = 1.0 + pu * pu
            curv = puu / (h * (gg * np.sqrt(gg)))
        curv = np.where(order == 2, curv, 0.0)
        l2 = g[:, 0] * g[:, 0]
        for d in range(1, D):
            l2 = l2 + g[:, d] * g[:, d]
        g = g / np.sqrt(l2)[:, None]
        if guide_normals is not None:
            G = NR._as_points(guide_normals, D).astype(np.float64)
            if G.shape[0] != n:
                raise ValueError("guide_normals: one per query")
            dot = _dot(g, G)
            flip = np.isfinite(dot) & (dot < 0.0)
            g = np.where(flip[:, None], -g, g)
            curv = np.where(flip, -curv, curv)
        # max_move: fi_mesh_smooth's rule
        dl = x1 - Q64
        s2 = dl[:, 0] * dl[:, 0] + dl[:, 1] * dl[:, 1]
        if D == 3:
            s2 = s2 + dl[:, 2] * dl[:, 2]
        far = s2 > mm * mm
        rr = mm / np.sqrt(s2)
        x1 = np.where(far[:, None], Q64 + dl * rr[:, None], x1)
        good = np.all(np.isfinite(x1), axis=1) & np.all(np.isfinite(g), axis=1) & np.isfinite(curv)
        stay = refused | ~good
        pos = np.where(stay[:, None], Q, x1.astype(np.float32))
        if queries is not None:                              # a non-finite query: NaN; a non-finite own point keeps its bits
            pos = np.where(np.all(np.isfinite(Q), axis=1)[:, None], pos, np.float32(np.nan))
        normals = np.where(stay[:, None], np.float32(0.0), g.astype(np.float32))
        curvature = np.where(stay, np.float32(np.nan), curv.astype(np.float32))
        order = np.where(stay, 0, order).astype(np.uint8)
    out = (pos.astype(np.float32), normals.astype(np.float32), curvature.astype(np.float32), order)
    if details:
        return out + ({"ratio": ratio, "m": m, "W": W},)
    return out
