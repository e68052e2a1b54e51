"""Numpy oracle of the nearest-point contract (include/fi_hip.h fi_nearest): a brute force over every
(query, point) pair in chunks, with the contract's fp32 arithmetic (s = 0 + (p_0 - q_0)^2 + ... in ascending axis order, one
rounding per operation), its tie rule (the smallest index), its max_distance rule and its non-finite rules.  Only numpy."""
import numpy as np


def _as_points(a, ndim):
    return np.ascontiguousarray(a, np.float32).reshape(-1, ndim)


def sq_dist(points, queries):
    """s (m, n) float32 of every (query, point) pair, in the contract's order of operations"""
    D = points.shape[1]
    s = np.zeros((queries.shape[0], points.shape[0]), np.float32)
    for d in range(D):
        e = points[None, :, d] - queries[:, None, d]          # float32 - float32: one rounding
        s = s + e * e                                          # float32 product, float32 sum
    return s


def nearest(points, queries, ndim, max_distance=np.inf, chunk_pairs=1 << 22):
    """(distances float32 (m,), indices int64 (m,)) of the nearest of `points` to each of `queries` (both x fastest)"""
    P = _as_points(points, ndim)
    Q = _as_points(queries, ndim)
    md = np.float32(max_distance)
    keep = np.flatnonzero(np.all(np.isfinite(P), axis=1))     # ascending: the first match is the smallest index
    Pf = P[keep]
    m = Q.shape[0]
    dist = np.full(m, np.inf, np.float32)
    idx = np.full(m, -1, np.int64)
    qok = np.all(np.isfinite(Q), axis=1)
    dist[~qok] = np.nan
    if Pf.shape[0] > 0:
        rows = np.flatnonzero(qok)
        step = max(1, chunk_pairs // Pf.shape[0])
        with np.errstate(over="ignore"):
            for b in range(0, rows.size, step):
                r = rows[b: b + step]
                s = sq_dist(Pf, Q[r])
                best = s.min(axis=1)
                first = np.argmax(s == best[:, None], axis=1)
                d = np.sqrt(best).astype(np.float32)
                far = d > md
                dist[r] = np.where(far, np.float32(np.inf), d)
                idx[r] = np.where(far, -1, keep[first])
    return dist, idx


def lattice_points(sizes):
    """every lattice point (x fastest) as float32 coordinates (N, D)"""
    grids = np.meshgrid(*[np.arange(s, dtype=np.float32) for s in sizes], indexing="ij")
    return np.stack([g.reshape(-1, order="F") for g in grids], axis=1) if len(sizes) > 1 else grids[0].reshape(-1, 1)


def distance_field(points, sizes, max_distance=np.inf):
    return nearest(points, lattice_points(sizes), len(sizes), max_distance)
