"""Numpy restatement of the contracts of fi_points_describe and fi_feature_match (include/fi_hip.h): fast
point feature histograms with a pseudo-angle, and the nearest descriptor of one set for every descriptor of another.  Test
infrastructure, independent of the device code.  Every floating-point step is written the way the contract states it -- fp64
from the fp32 positions and normals (fp32 in the matching), one rounding per operation, every sum in its stated order -- so
that every float returned is the bit pattern the device must produce.  Only numpy and normals_reference.knn."""
import numpy as np

import normals_reference as N

WIDTH, BINS = 33, 11


class Invalid(Exception):
    """what the device answers with FI_ERR_INVALID"""


class Unsupported(Exception):
    """what the device answers with FI_ERR_UNSUPPORTED"""


def dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], axis=-1)


def live_points(P32, N32):
    """(live (n,), unit normals float64 (n, 3), zeros where not live)"""
    nrm = N32.astype(np.float64)
    with np.errstate(all="ignore"):
        length = np.sqrt(dot(nrm, nrm))
        live = np.all(np.isfinite(P32), axis=1) & np.all(np.isfinite(N32), axis=1) & np.isfinite(length) & (length > 0.0)
        unit = np.where(live[:, None], nrm / length[:, None], 0.0)
    return live, unit


def bins(t):
    with np.errstate(invalid="ignore"):
        return np.where(t < 0.0, 0, np.where(t >= 11.0, 10, np.where(np.isfinite(t), t, 0.0).astype(np.int64)))


def pair_features(P, unit, i, j):
    """(f (p, 3), counted (p,), w (p,)) of the pairs (i, j) (index arrays): the three features, whether the pair is counted,
    and the squared distance"""
    with np.errstate(all="ignore"):
        dp = P[j] - P[i]
        w = dot(dp, dp)
        L = np.sqrt(w)
        e = dp / L[:, None]
        ni, nj = unit[i], unit[j]
        ai, aj = dot(ni, e), dot(nj, e)
        swap = np.abs(ai) < np.abs(aj)
        ns = np.where(swap[:, None], nj, ni)
        nt = np.where(swap[:, None], ni, nj)
        e = np.where(swap[:, None], -e, e)
        f2 = np.where(swap, -aj, ai)
        v = cross(e, ns)
        l = np.sqrt(dot(v, v))
        ok = np.isfinite(l) & (l > 0.0)
        v = v / l[:, None]
        u = cross(ns, v)
        f1, x, y = dot(v, nt), dot(ns, nt), dot(u, nt)
        s = np.abs(x) + np.abs(y)
        r = np.where(s > 0.0, y / s, 0.0)
        f3 = np.where(x >= 0.0, r, np.where(y >= 0.0, 2.0 - r, -2.0 - r))
        f = np.stack([f1, f2, f3], axis=1)
        ok &= np.all(np.isfinite(f), axis=1)
    return f, ok, w


def describe(points, normals, k=32, max_distance=np.inf, ndim=3, neighbours=None, parts=False):
    """-> (features float32 (n, 33), valid uint8 (n,)); neighbours: the indices of normals_reference.knn(points, points, 3, k,
    max_distance); parts=True also returns the integer counts c (n, 33) and m (n,)"""
    if points is None or normals is None:
        raise Invalid("null")
    if not 1 <= k <= N.MAX_K:
        raise Invalid("k")
    if not np.float32(max_distance) >= 0:
        raise Invalid("max_distance")
    if ndim != 3:
        raise Unsupported("ndim")
    P32 = np.asarray(points, np.float32).reshape(-1, 3)
    N32 = np.asarray(normals, np.float32).reshape(-1, 3)
    n = len(P32)
    feat, valid = np.zeros((n, WIDTH), np.float32), np.zeros(n, np.uint8)
    c, m = np.zeros((n, WIDTH), np.int64), np.zeros(n, np.int64)
    if n == 0:
        return (feat, valid, c, m) if parts else (feat, valid)
    idx = neighbours if neighbours is not None else N.knn(P32, P32, 3, k, max_distance)[1]
    P = P32.astype(np.float64)
    live, unit = live_points(P32, N32)
    # the neighbour entries of every point, row by row in result order
    i = np.repeat(np.arange(n, dtype=np.int64), idx.shape[1])
    j = idx.reshape(-1)
    keep = (j >= 0) & (j != i) & live[i] & live[np.where(j >= 0, j, 0)]
    i, j = i[keep], j[keep]
    f, counted, w = pair_features(P, unit, i, j)
    near = w != 0.0                                    # the neighbours of item 2: the duplicates are gone
    i, j, f, counted, w = i[near], j[near], f[near], counted[near], w[near]
    b = np.stack([bins((f[:, 0] + 1.0) * 5.5), BINS + bins((f[:, 1] + 1.0) * 5.5), 2 * BINS + bins((f[:, 2] + 2.0) * 2.75)], axis=1)
    for col in range(3):
        np.add.at(c, (i[counted], b[counted, col]), 1)
    np.add.at(m, i[counted], 1)
    has = live & (m > 0)
    with np.errstate(all="ignore"):
        S = np.where(has[:, None], (100.0 * c.astype(np.float64)) / m.astype(np.float64)[:, None], 0.0)
    # the weighted sum over the neighbours with a descriptor of their own, in result order: one entry after the other
    A, q = np.zeros((n, WIDTH)), np.zeros(n, np.int64)
    use = has[i] & has[j]
    i, j, w = i[use], j[use], w[use]
    rank = np.zeros(len(i), np.int64)                  # the position of an entry among its point's entries
    if len(i):
        start = np.flatnonzero(np.concatenate([[True], i[1:] != i[:-1]]))
        rank = np.arange(len(i)) - np.repeat(start, np.diff(np.concatenate([start, [len(i)]])))
    for step in range(int(rank.max()) + 1 if len(i) else 0):
        at = rank == step
        A[i[at]] = A[i[at]] + S[j[at]] / w[at, None]
        q[i[at]] += 1
    with np.errstate(all="ignore"):
        F = S + np.where(q[:, None] > 0, A / q.astype(np.float64)[:, None], 0.0)
        for blk in range(3):
            z = np.zeros(n)
            for col in range(blk * BINS, (blk + 1) * BINS):
                z = z + F[:, col]
            cols = slice(blk * BINS, (blk + 1) * BINS)
            F[:, cols] = np.where(z[:, None] > 0.0, (100.0 * F[:, cols]) / z[:, None], F[:, cols])
    feat[has] = F[has].astype(np.float32)
    valid[has] = 1
    return (feat, valid, c, m) if parts else (feat, valid)


def match(a, b, valid_a=None, valid_b=None, dim=None):
    """-> (indices int64 (n_a,), distances float32 (n_a,)): the smallest j with the minimal fp32 sum of squared differences
    over ascending columns, among the valid, finite rows of b; -1 and +inf for an invalid or non-finite row of a or no such j"""
    a32, b32 = np.asarray(a, np.float32), np.asarray(b, np.float32)
    dim = a32.shape[1] if dim is None else dim
    if not 1 <= dim <= 64:
        raise Invalid("dim")
    a32, b32 = a32.reshape(-1, dim), b32.reshape(-1, dim)
    na, nb = len(a32), len(b32)
    oka = np.all(np.isfinite(a32), axis=1) & (np.ones(na, bool) if valid_a is None else np.asarray(valid_a).astype(np.uint8) != 0)
    okb = np.all(np.isfinite(b32), axis=1) & (np.ones(nb, bool) if valid_b is None else np.asarray(valid_b).astype(np.uint8) != 0)
    idx, dist = np.full(na, -1, np.int64), np.full(na, np.inf, np.float32)
    rows, cand = np.flatnonzero(oka), np.flatnonzero(okb)
    if len(rows) == 0 or len(cand) == 0:
        return idx, dist
    B = b32[cand]
    step = max(1, (1 << 22) // len(cand))
    with np.errstate(over="ignore"):
        for lo in range(0, len(rows), step):
            r = rows[lo:lo + step]
            s = np.zeros((len(r), len(cand)), np.float32)
            for col in range(dim):
                d = a32[r, col, None] - B[None, :, col]
                s = s + d * d
            at = np.argmin(s, axis=1)                   # the first of equal minima: the smallest j
            idx[r] = cand[at]
            dist[r] = np.sqrt(s[np.arange(len(r)), at])
    return idx, dist


def match_mutual(a, b, valid_a=None, valid_b=None):
    """match(a, b) with -1 (and +inf) where the match of b's row does not come back"""
    idx, dist = match(a, b, valid_a, valid_b)
    back, _ = match(b, a, valid_b, valid_a)
    lost = (idx >= 0) & (back[np.where(idx >= 0, idx, 0)] != np.arange(len(idx)))
    idx[lost], dist[lost] = -1, np.inf
    return idx, dist
