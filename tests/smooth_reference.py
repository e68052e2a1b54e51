"""Numpy restatement of the mesh-smoothing contract (include/fi_hip.h fi_mesh_smooth / fi_mesh_normals): Taubin
fairing with uniform weights and normals recomputed from the primitives.  Test infrastructure, independent of the device code.
Every floating-point step is written the way the contract states it -- fp64 from the fp32 coordinates, one rounding per
operation, every sum serial from 0 in ascending order -- so that the arrays returned are the bytes the device must produce.
The ordered sums are vectorised by rank: pass k adds every row's k-th entry, which is the same serial order for every row
(tests/test_smooth_reference.py holds that against a plain per-vertex loop)."""
import numpy as np

FIXED, SLIDE, FREE = 0, 1, 2
RECOMPUTE, KEEP = 0, 1
BOUNDARY = {"fixed": FIXED, "slide": SLIDE, "free": FREE}
NORMALS = {"recompute": RECOMPUTE, "keep": KEEP}


class Invalid(Exception):
    """what the device answers with FI_ERR_INVALID"""


def _rows(indices, D):
    return np.asarray(indices, np.int64).reshape(-1, D)


def half_edges(idx):
    """the half-edges of fi_mesh_parts, those with equal ends left out -> int64 (n, 2)"""
    D = idx.shape[1]
    he = np.concatenate([idx[:, [0, 1]], idx[:, [1, 2]], idx[:, [2, 0]]]) if D == 3 else idx[:, [0, 1]]
    return he[he[:, 0] != he[:, 1]]


def adjacency(nv, indices, D):
    """-> (v, w, edge_is_boundary, vertex_is_boundary): the distinct directed pairs (v, w) with w in N(v), sorted by (v, w),
    whether the pair is a boundary edge (3-D; all False in 2-D), and per vertex whether it is a boundary vertex"""
    he = half_edges(_rows(indices, D))
    both = np.concatenate([he, he[:, ::-1]])
    key, cnt = np.unique(both[:, 0] * (nv + 1) + both[:, 1], return_counts=True)
    v, w = key // (nv + 1), key % (nv + 1)
    vb = np.zeros(nv, bool)
    if D == 3:
        eb = cnt == 1                                   # the unordered pair is used by exactly one half-edge
        vb[v[eb]] = True
    else:
        eb = np.zeros(len(key), bool)
        vb = np.bincount(both[:, 0], minlength=nv) == 1  # total degree 1
    return v, w, eb, vb


def rows(nv, indices, D, boundary):
    """The set every vertex averages over, as a CSR (offsets int64 (nv + 1,), neighbours int64), ascending within a row; an
    empty row: the vertex never moves."""
    v, w, eb, vb = adjacency(nv, indices, D)
    if boundary == FREE:
        keep = np.ones(len(v), bool)
    elif boundary == FIXED or D == 2:
        keep = ~vb[v]
    else:
        keep = ~vb[v] | eb
    v, w = v[keep], w[keep]
    off = np.zeros(nv + 1, np.int64)
    np.cumsum(np.bincount(v, minlength=nv), out=off[1:])
    return off, w


def ranked_sum(off, nbr, x):
    """s_v = the serial sum from 0 of x[nbr] over row v, in row order -> float64 (nv, D)"""
    deg = np.diff(off)
    s = np.zeros((len(deg), x.shape[1]), np.float64)
    for k in range(int(deg.max()) if len(deg) else 0):
        on = deg > k
        s[on] = s[on] + x[nbr[off[:-1][on] + k]]
    return s


def step(off, nbr, x, f):
    deg = np.diff(off)
    on = deg > 0
    s = ranked_sum(off, nbr, x)
    out = x.copy()
    avg = s[on] / deg[on].astype(np.float64)[:, None]
    t = avg - x[on]
    t = np.float64(f) * t
    out[on] = x[on] + t
    return out


def clamp(x, x0, m):
    d = x - x0
    s2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    if x.shape[1] == 3:
        s2 = s2 + d[:, 2] * d[:, 2]
    over = s2 > m * m
    out = x.copy()
    with np.errstate(all="ignore"):
        out[over] = (x0 + d * (m / np.sqrt(s2))[:, None])[over]
    return out


def _check_finite(pos, idx):
    used = np.zeros(len(pos), bool)
    used[idx.reshape(-1)] = True
    if not np.all(np.isfinite(pos[used])):
        raise Invalid("a non-finite coordinate of a used vertex")


def primitive_normals(pos, idx):
    """n_p in fp64 from the fp32 positions: 3-D (b - a) x (c - a), 2-D (e_y, -e_x) with e = b - a"""
    p = pos.astype(np.float64)
    a, b = p[idx[:, 0]], p[idx[:, 1]]
    if idx.shape[1] == 3:
        u, w = b - a, p[idx[:, 2]] - a
        return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                         u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
    e = b - a
    return np.stack([e[:, 1], -e[:, 0]], axis=1)


def mesh_normals(vertices, indices):
    """-> float32 (V, D): every vertex's primitives in ascending number (one that names it twice counts once), their n_p summed,
    the sum divided by its length; zeros for a zero sum and for an unused vertex"""
    pos = np.asarray(vertices, np.float32)
    D = pos.shape[1]
    idx = _rows(indices, D)
    nv = len(pos)
    if len(idx) == 0:
        return np.zeros((nv, D), np.float32)
    _check_finite(pos, idx)
    n = primitive_normals(pos, idx)
    vs, ps = [], []
    for k in range(D):
        new = np.ones(len(idx), bool)
        for j in range(k):
            new &= idx[:, k] != idx[:, j]
        vs.append(idx[new, k])
        ps.append(np.flatnonzero(new))
    vs, ps = np.concatenate(vs), np.concatenate(ps)
    order = np.lexsort((ps, vs))                       # by vertex, ascending primitive within one
    vs, ps = vs[order], ps[order]
    off = np.zeros(nv + 1, np.int64)
    np.cumsum(np.bincount(vs, minlength=nv), out=off[1:])
    s = ranked_sum(off, ps, n)
    l2 = s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]
    if D == 3:
        l2 = l2 + s[:, 2] * s[:, 2]
    ln = np.sqrt(l2)
    with np.errstate(all="ignore"):
        return np.where(ln[:, None] > 0.0, s / ln[:, None], 0.0).astype(np.float32)


def smooth(vertices, normals, indices, iterations=10, lam=0.5, mu=-0.53, boundary=FIXED, max_move=0.0, normals_mode=RECOMPUTE):
    """-> (vertices float32 (V, D), normals float32 (V, D) or None).  One iteration: a lambda step, a mu step if mu != 0, then
    -- once, behind the iteration's last step -- the clamp to max_move of the input position if max_move > 0."""
    pos = np.asarray(vertices, np.float32)
    D = pos.shape[1]
    idx = _rows(indices, D)
    lam, mu, max_move = np.float32(lam), np.float32(mu), np.float32(max_move)
    if (iterations < 0 or not (0 <= lam <= 1) or not (-2 <= mu <= 0) or not (max_move >= 0)
            or boundary not in (FIXED, SLIDE, FREE) or normals_mode not in (RECOMPUTE, KEEP)):
        raise Invalid("options")
    if len(idx):
        _check_finite(pos, idx)
    out = pos.copy()
    if iterations > 0 and len(idx):
        off, nbr = rows(len(pos), idx, D, boundary)
        x0 = pos.astype(np.float64)
        x = x0
        for _ in range(iterations):
            x = step(off, nbr, x, lam)
            if mu != 0:
                x = step(off, nbr, x, mu)
            if max_move > 0:
                x = clamp(x, x0, np.float64(max_move))
        out = x.astype(np.float32)
    if normals is None:
        return out, None
    if normals_mode == KEEP:
        return out, np.asarray(normals, np.float32).copy()
    return out, mesh_normals(out, idx)
