"""Numpy restatement of the mesh-simplification contract (include/fi_hip.h fi_mesh_simplify): vertex
clustering on a uniform grid with each cluster's vertex placed by its quadric (or at its mean).  Test infrastructure,
independent of the device code.  Every floating-point step is written the way the contract states it -- fp32 for the cell of
a vertex, fp64 with one rounding per operation for everything else, every sum serial in ascending order (np.add.at adds one
entry after the other) -- so that the arrays returned are the bytes the device must produce.  Only numpy (and the Jacobi
iteration of normals_reference, which the normal estimation already defines)."""
import numpy as np

import normals_reference as NR

QUADRIC, MEAN = 0, 1
BIAS = 1 << 20
RANK_TOLERANCE = 1e-3


class Invalid(Exception):
    """what the device answers with FI_ERR_INVALID"""


class Result:
    """vertices (V, D) float32, normals (V, D) float32 or None, indices (P, D) int32, keys (V,) int64, vertex_map (input
    vertices,) int32; clusters: how many there were; fallbacks: the output vertices whose quadric minimiser was refused"""

    def __init__(self, vertices, normals, indices, keys, vertex_map, clusters=0, fallbacks=0):
        self.vertices, self.normals, self.indices, self.keys, self.vertex_map = vertices, normals, indices, keys, vertex_map
        self.clusters, self.fallbacks = clusters, fallbacks


def _rows(indices, D):
    a = np.asarray(indices, np.int64)
    return a.reshape(-1, D)


def cell_keys(vertices, cell, origin):
    """(cells int64 (n, D), keys int64 (n,)) of the vertices given: c = floorf((p - o) / cell) in fp32"""
    p = np.asarray(vertices, np.float32)
    D = p.shape[1]
    if not np.all(np.isfinite(p)):
        raise Invalid("a non-finite coordinate")
    with np.errstate(all="ignore"):
        c = np.floor((p - origin[None, :]) / np.float32(cell))
    assert c.dtype == np.float32
    if not np.all(np.abs(c) < np.float32(BIAS)):      # (a NaN fails the comparison too)
        raise Invalid("a cell beyond 2^20")
    c = c.astype(np.int64)
    key = np.zeros(len(p), np.int64)
    for a in range(D):
        key |= (c[:, a] + BIAS) << (21 * a)
    return c, key


def canonical(t):
    """the oriented tuples of the rows of t (n, D): 3-D rotated so that the smallest index comes first, 2-D as they are"""
    if t.shape[1] == 2 or len(t) == 0:
        return t
    first = np.argmin(t, axis=1)                       # (the first of equal minima: only degenerate rows have them)
    r = np.arange(len(t))
    return np.stack([t[r, first], t[r, (first + 1) % 3], t[r, (first + 2) % 3]], axis=1)


def cluster_sums(rel, normals_of, members, cluster_of, K):
    """x-bar sums, counts and normal sums of the clusters: members ascending, one after the other"""
    D = rel.shape[1]
    s = np.zeros((K, D), np.float64)
    np.add.at(s, cluster_of, rel)
    cnt = np.bincount(cluster_of, minlength=K).astype(np.float64)
    ns = None
    if normals_of is not None:
        ns = np.zeros((K, D), np.float64)
        np.add.at(ns, cluster_of, normals_of)
    return s, cnt, ns


def primitive_terms(idx, pos64, vcl, g):
    """Every (primitive, distinct cluster among its vertices) pair in ascending primitive number -> (cluster (m,), A terms
    (m, D, D), b terms (m, D)): the primitive's normal n from its vertices relative to that cluster's centre, n n^T and
    n (n . a')"""
    D = idx.shape[1]
    t = vcl[idx]
    cl, pr = [], []
    for k in range(D):
        new = np.ones(len(idx), bool)
        for j in range(k):
            new &= t[:, k] != t[:, j]
        cl.append(t[new, k])
        pr.append(np.flatnonzero(new))
    cl, pr = np.concatenate(cl), np.concatenate(pr)
    order = np.argsort(pr, kind="stable")              # ascending primitive (a primitive's clusters differ: their order is free)
    cl, pr = cl[order], pr[order]
    gc = g[cl]
    a = pos64[idx[pr, 0]] - gc
    b = pos64[idx[pr, 1]] - gc
    if D == 3:
        c = pos64[idx[pr, 2]] - gc
        u, w = b - a, c - a
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                      u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
        na = (n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2]
    else:
        e = b - a
        n = np.stack([-e[:, 1], e[:, 0]], axis=1)
        na = n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]
    return cl, n[:, :, None] * n[:, None, :], n * na[:, None]


def minimise(A, b, xbar, cell):
    """x' of every cluster and whether it fell back to x-bar"""
    K, D = xbar.shape
    lam, V = NR.jacobi(A)
    lmax = lam.max(axis=1)
    Ax = A[:, :, 0] * xbar[:, None, 0]
    for d in range(1, D):
        Ax = Ax + A[:, :, d] * xbar[:, None, d]
    r = b - Ax
    x = xbar.copy()
    with np.errstate(all="ignore"):
        for i in range(D):
            dot = V[:, 0, i] * r[:, 0]
            for d in range(1, D):
                dot = dot + V[:, d, i] * r[:, d]
            coef = dot / lam[:, i]
            on = (lmax > 0.0) & (lam[:, i] > RANK_TOLERANCE * lmax)
            x = np.where(on[:, None], x + V[:, :, i] * coef[:, None], x)
        bad = ~np.all(np.isfinite(x), axis=1) | np.any(np.abs(x) > np.float64(np.float32(cell)), axis=1)
    return np.where(bad[:, None], xbar, x), bad


def simplify(vertices, normals, indices, cell, origin=None, placement=QUADRIC):
    """-> Result.  vertices (V, D) float32, normals (V, D) float32 or None, indices (P, D)."""
    pos = np.asarray(vertices, np.float32)
    D = pos.shape[1]
    pos = pos.reshape(-1, D)
    idx = _rows(indices, D)
    nrm = None if normals is None else np.asarray(normals, np.float32).reshape(-1, D)
    cell = np.float32(cell)
    if not cell > 0 or placement not in (QUADRIC, MEAN):
        raise Invalid("cell or placement")
    o = np.zeros(D, np.float32) if origin is None else np.asarray(origin, np.float32).reshape(D)
    nv = len(pos)
    vmap = np.full(nv, -1, np.int32)
    empty = Result(np.zeros((0, D), np.float32), None if nrm is None else np.zeros((0, D), np.float32), np.zeros((0, D), np.int32),
                   np.zeros(0, np.int64), vmap)
    if len(idx) == 0 or nv == 0:
        return empty
    used = np.zeros(nv, bool)
    used[idx.reshape(-1)] = True
    members = np.flatnonzero(used)                     # ascending
    cells, keys = cell_keys(pos[members], cell, o)
    ckeys, first, cluster_of = np.unique(keys, return_index=True, return_inverse=True)
    K = len(ckeys)
    vcl = np.full(nv, -1, np.int64)
    vcl[members] = cluster_of
    g = o.astype(np.float64)[None, :] + (cells[first].astype(np.float64) + 0.5) * np.float64(cell)

    # primitives: cluster numbers, degenerates out, the lowest of every oriented tuple
    t = vcl[idx]
    degenerate = t[:, 0] == t[:, 1]
    if D == 3:
        degenerate |= (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])
    alive = np.flatnonzero(~degenerate)
    _, low = np.unique(canonical(t[alive]), axis=0, return_index=True) if len(alive) else (None, np.empty(0, np.int64))
    kept = alive[np.sort(low)]
    out_of = np.zeros(K, bool)
    out_of[t[kept].reshape(-1)] = True
    number = np.cumsum(out_of) - 1
    vmap[members] = np.where(out_of[cluster_of], number[cluster_of], -1).astype(np.int32)
    if len(kept) == 0:
        empty.clusters = K
        return empty

    # placement
    pos64 = pos.astype(np.float64)
    rel = pos64[members] - g[cluster_of]
    s, cnt, ns = cluster_sums(rel, None if nrm is None else nrm[members].astype(np.float64), members, cluster_of, K)
    xbar = s / cnt[:, None]
    bad = np.zeros(K, bool)
    x = xbar
    if placement == QUADRIC:
        cl, At, bt = primitive_terms(idx, pos64, vcl, g)
        A = np.zeros((K, D, D), np.float64)
        b = np.zeros((K, D), np.float64)
        np.add.at(A, cl, At)
        np.add.at(b, cl, bt)
        x, bad = minimise(A, b, xbar, cell)
    out_pos = (g + x).astype(np.float32)[out_of]
    out_nrm = None
    if nrm is not None:
        l2 = ns[:, 0] * ns[:, 0]
        for d in range(1, D):
            l2 = l2 + ns[:, d] * ns[:, d]
        ln = np.sqrt(l2)
        with np.errstate(all="ignore"):
            out_nrm = np.where(ln[:, None] > 0.0, ns / ln[:, None], 0.0).astype(np.float32)[out_of]
    return Result(out_pos, out_nrm, number[t[kept]].astype(np.int32), ckeys[out_of].astype(np.int64), vmap, K, int(bad[out_of].sum()))


# ---- the meshes of the tests ------------------------------------------------------------------------------------------

def cube_mesh(n=12, lo=2.25, h=0.75):
    """The exactly tessellated cube [lo, lo + n h]^3: n x n quads a face, two triangles each, outward, vertices shared
    -> (vertices float32, indices int32)"""
    ids = {}
    verts, tris = [], []

    def vid(i, j, k):
        if (i, j, k) not in ids:
            ids[(i, j, k)] = len(verts)
            verts.append((lo + i * h, lo + j * h, lo + k * h))
        return ids[(i, j, k)]

    for axis in range(3):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for u in range(n):
                for v in range(n):
                    def at(du, dv):
                        q = [0, 0, 0]
                        q[axis], q[b], q[c] = side, u + du, v + dv
                        return vid(*q)
                    q0, q1, q2, q3 = at(0, 0), at(1, 0), at(1, 1), at(0, 1)    # normal +axis
                    quad = (q0, q1, q2, q3) if side else (q0, q3, q2, q1)
                    tris.append((quad[0], quad[1], quad[2]))
                    tris.append((quad[0], quad[2], quad[3]))
    return np.asarray(verts, np.float32), np.asarray(tris, np.int32)


def sphere_field(n=24, radius=9.0, centre=None):
    """distance to a sphere on n^3, fp32, flat (x fastest)"""
    c = [(n - 1) / 2.0 + 0.13, (n - 1) / 2.0 - 0.21, (n - 1) / 2.0 + 0.07] if centre is None else centre
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij")
    return (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - radius).astype(np.float32).reshape(-1), c


def soup(vertices, indices, normals=None):
    """every primitive with vertices of its own"""
    idx = np.asarray(indices).reshape(-1)
    out = np.arange(len(idx), dtype=np.int32).reshape(np.asarray(indices).shape)
    return np.asarray(vertices)[idx], out, None if normals is None else np.asarray(normals)[idx]


def square_polyline(n=8, lo=1.5, h=0.5):
    """the boundary of the square [lo, lo + n h]^2 as 4 n segments, counter-clockwise (the inside on the left)"""
    pts = [(lo + i * h, lo) for i in range(n)] + [(lo + n * h, lo + i * h) for i in range(n)] + \
          [(lo + (n - i) * h, lo + n * h) for i in range(n)] + [(lo, lo + (n - i) * h) for i in range(n)]
    m = len(pts)
    return np.asarray(pts, np.float32), np.asarray([(i, (i + 1) % m) for i in range(m)], np.int32)
