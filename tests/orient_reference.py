"""Numpy oracle of the normal-orientation contract (include/fi_hip.h fi_orient_normals): the neighbour graph
of the live points from normals_reference.knn, its edges valued by the agreement of the normal lines (fp64 from the fp32
normals, one rounding per operation), the unique minimum spanning forest under the strict order (a descending, lo
ascending, hi ascending) by Kruskal's algorithm over the sorted edge list with a union-find that carries each vertex's
parity, and the sign of every component from the extreme rule or the guides' vote.  Only numpy."""
import numpy as np

import nearest_reference as R
import normals_reference as N


def live_points(P, nrm):
    """position finite, normal finite and not all zeros"""
    return np.all(np.isfinite(P), axis=1) & np.all(np.isfinite(nrm), axis=1) & np.any(nrm != 0, axis=1)


def edges(nrm, idx, live):
    """(lo, hi, a float32, flip bool) of the undirected edges, each once, in the contract's order"""
    n, k = idx.shape
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    j = idx.reshape(-1)
    ok = (j >= 0) & (j != i) & live[i] & live[np.where(j >= 0, j, 0)]
    i, j = i[ok], j[ok]
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    pair = np.unique(np.stack([lo, hi], 1), axis=0)
    lo, hi = pair[:, 0], pair[:, 1]
    a64 = nrm.astype(np.float64)
    d = np.zeros(lo.size, np.float64)
    with np.errstate(all="ignore"):
        for ax in range(nrm.shape[1]):
            d = d + a64[lo, ax] * a64[hi, ax]
        a = np.abs(d).astype(np.float32)
    order = np.lexsort((hi, lo, -a.astype(np.float64)))              # the last key is the primary one
    return lo[order], hi[order], a[order], (d < 0)[order]


def forest_signs(n, lo, hi, flip):
    """Kruskal over the sorted edges: (root of each vertex, parity of each vertex relative to its root, forest edge mask)"""
    parent = list(range(n))
    par = [0] * n

    def find(v):
        path = []
        while parent[v] != v:
            path.append(v)
            v = parent[v]
        acc = 0
        for u in reversed(path):                                     # from the vertex next to the root outwards
            acc ^= par[u]
            parent[u], par[u] = v, acc
        return v

    taken = np.zeros(lo.size, bool)
    for e, (u, v, f) in enumerate(zip(lo.tolist(), hi.tolist(), flip.tolist())):
        ru, rv = find(u), find(v)
        if ru == rv:
            continue
        taken[e] = True
        parent[ru] = rv                                              # t_ru relative to rv: t_u t_v = -1 exactly with flip
        par[ru] = par[u] ^ par[v] ^ int(f)
    roots = np.array([find(v) for v in range(n)], np.int64)
    return roots, np.array(par, np.int64), taken


def vote_weights(P, nrm, viewpoints, directions):
    """w of fi_estimate_normals step 5 for the given normals, or None without guides"""
    n, D = P.shape
    if viewpoints is None and directions is None:
        return None
    P64 = P.astype(np.float64)
    with np.errstate(all="ignore"):
        if viewpoints is not None:
            v = R._as_points(viewpoints, D).astype(np.float64)
            if v.shape[0] not in (1, n):
                raise ValueError("viewpoints: one, or one per point")
            g = np.broadcast_to(v, (n, D)) - P64
        else:
            g = R._as_points(directions, D).astype(np.float64)
            if g.shape[0] != n:
                raise ValueError("directions: one per point")
        w = np.zeros(n, np.float64)
        for a in range(D):
            w = w + nrm[:, a].astype(np.float64) * g[:, a]
    return w


def extreme_sign(P, nrm, t, members):
    """Hoppe's rule: the member highest on the last axis (fp32, the smallest index on a tie) looks along that axis"""
    D = P.shape[1]
    top = P[members, D - 1]
    e = members[np.flatnonzero(top == top.max())[0]]
    for ax in range(D - 1, -1, -1):
        c = nrm[e, ax]
        if c != 0:
            return -1 if (c < 0) != (t[e] < 0) else 1
    return 1


def orient_normals(points, normals, ndim, k, max_distance=np.inf, viewpoints=None, directions=None, neighbours=None):
    """(normals float32 (n, D), components int64 (n,)): `normals` with a consistent sign per connected component of the
    k-nearest-neighbour graph; neighbours: the (distances, indices) of knn(points, points, ndim, k, max_distance)"""
    if ndim < 2:
        raise ValueError("normals need 2 or 3 dimensions")
    if viewpoints is not None and directions is not None:
        raise ValueError("viewpoints or directions, not both")
    P = R._as_points(points, ndim)
    nrm = np.array(R._as_points(normals, ndim), np.float32)
    n, D = P.shape
    comp = np.full(n, -1, np.int64)
    if n == 0:
        return nrm, comp
    _, idx = neighbours if neighbours is not None else N.knn(P, P, D, k, max_distance)
    live = live_points(P, nrm)
    lo, hi, _, flip = edges(nrm, idx, live)
    roots, par, _ = forest_signs(n, lo, hi, flip)
    w = vote_weights(P, nrm, viewpoints, directions)
    t = np.ones(n, np.int64)
    out = nrm.copy()
    order = np.argsort(roots, kind="stable")
    cuts = np.flatnonzero(np.diff(roots[order])) + 1
    for members in np.split(order, cuts):                            # ascending indices within a component
        if not live[members[0]]:
            continue
        c = members[0]
        t[members] = np.where(par[members] == par[c], 1, -1)
        comp[members] = c
        S = 0
        if w is not None:
            wm = w[members] * t[members]
            plus = int(np.sum(np.isfinite(wm) & (wm > 0)))
            minus = int(np.sum(np.isfinite(wm) & (wm < 0)))
            S = 1 if plus > minus else (-1 if minus > plus else 0)
        if S == 0:
            S = extreme_sign(P, nrm, t, members)
        neg = members[t[members] * S < 0]
        out[neg] = -nrm[neg]
    return out, comp
