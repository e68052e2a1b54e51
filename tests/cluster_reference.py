"""Numpy restatement of the point-cloud clustering contract (include/fi_hip.h fi_cluster .. fi_cluster_measure; DESIGN.md
4.20): the definition the device is held to bit for bit.  Brute force over every pair with nearest_reference.sq_dist's fp32
arithmetic (cloud_reference's order of operations), a serial union-find over the pairs in ascending order, the border rule as
a search for the first (s, j) over the core points, and meshpts_reference.tree_sum for the chunked centroid.  It shares
nothing with the device path: no tree, no Morton order, no atomics.  Only numpy."""
import numpy as np

import nearest_reference as NR
from cloud_reference import _chunks, _finite
from meshpts_reference import tree_sum


def _within(Pf, rows, eps32):
    """(s float32 (len(rows), nf), s within eps) of the finite points `rows` against every finite point"""
    with np.errstate(over="ignore"):
        s = NR.sq_dist(Pf, Pf[rows])
        return s, np.sqrt(s) <= eps32


def cluster(points, ndim, eps, min_points=1):
    """-> (labels int32 (n,), core uint8 (n,), stats dict: clusters, core, border, noise, non_finite)"""
    if not (eps >= 0.0 and np.isfinite(eps)):
        raise ValueError("eps must be finite and >= 0")
    if min_points < 1:
        raise ValueError("min_points must be >= 1")
    P = NR._as_points(points, ndim)
    n = P.shape[0]
    eps32 = np.float32(eps)
    idx = np.flatnonzero(_finite(P))                          # ascending: positions among them order like indices
    Pf = P[idx]
    nf = idx.size
    every = np.arange(nf)
    is_core = np.zeros(nf, bool)
    for r in _chunks(every, nf):                              # the count includes the point itself
        is_core[r] = _within(Pf, r, eps32)[1].sum(axis=1) >= min_points
    # the serial union over the pairs of core points within eps, in ascending order; a root is its set's smallest member
    parent = np.arange(nf)

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    cores = np.flatnonzero(is_core)
    for r in _chunks(cores, nf):
        near = _within(Pf, r, eps32)[1] & is_core[None, :]
        a, b = np.nonzero(near)
        for i, j in zip(r[a], b):
            if j < i:
                ri, rj = find(i), find(j)
                if ri != rj:
                    parent[max(ri, rj)] = min(ri, rj)
    root = np.array([find(v) for v in every], np.int64) if nf else np.zeros(0, np.int64)
    roots = np.flatnonzero(is_core & (root == every))         # ascending: the lowest core point numbers the cluster
    number = np.full(nf, -1, np.int64)
    number[roots] = np.arange(roots.size)
    label_f = np.full(nf, -1, np.int64)
    label_f[is_core] = number[root[is_core]]
    # a point that is not core: the first (s, j) over the core points within eps
    others = np.flatnonzero(~is_core)
    border = 0
    if cores.size:
        for r in _chunks(others, nf):
            s, near = _within(Pf, r, eps32)
            near &= is_core[None, :]
            for k, i in enumerate(r):
                cand = np.flatnonzero(near[k])
                if cand.size:
                    best = s[k, cand].min()
                    j = cand[np.argmax(s[k, cand] == best)]   # the smallest index that reaches it
                    label_f[i] = number[root[j]]
                    border += 1
    labels = np.full(n, -1, np.int32)
    labels[idx] = label_f
    core = np.zeros(n, np.uint8)
    core[idx] = is_core
    stats = {"clusters": int(roots.size), "core": int(is_core.sum()), "border": border,
             "noise": int(nf - is_core.sum() - border), "non_finite": int(n - nf)}
    return labels, core, stats


def measure(positions, ndim, labels, core, num_clusters):
    """-> rows: a list of dicts count, core, lo float32 (3,), hi float32 (3,), centroid float64 (3,)"""
    P = NR._as_points(positions, ndim)
    L = np.asarray(labels, np.int64).reshape(-1)
    if np.any((L < -1) | (L >= num_clusters)):
        raise ValueError("a label lies outside [-1, num_clusters)")
    rows = []
    for c in range(num_clusters):
        members = np.flatnonzero(L == c)                      # ascending index
        row = {"count": int(members.size), "core": 0, "lo": np.zeros(3, np.float32), "hi": np.zeros(3, np.float32),
               "centroid": np.zeros(3, np.float64)}
        if members.size:
            if core is not None:
                row["core"] = int(np.count_nonzero(np.asarray(core).reshape(-1)[members]))
            for a in range(ndim):
                x = P[members, a]
                row["lo"][a], row["hi"][a] = x.min(), x.max()
                with np.errstate(over="ignore", invalid="ignore"):
                    row["centroid"][a] = tree_sum(x.astype(np.float64)) / np.float64(members.size)
        rows.append(row)
    return rows


def keep(rows, largest=None, min_points=0):
    """the clusters with at least min_points members; with largest = k only the k largest of them (ties: the lower number)"""
    count = np.array([r["count"] for r in rows], np.int64)
    mask = count >= int(min_points)
    if largest is not None:
        order = np.argsort(-count, kind="stable")
        order = order[mask[order]][:int(largest)]
        mask = np.zeros(len(rows), bool)
        mask[order] = True
    return mask


def clump_cloud(seed, n=1500, clump=30, away=5.0):
    """the sphere scan of the tests (util.sphere_points in a 32^3 lattice, radius 9.3) with a planted clump: `clump` points in
    a ball of radius 0.8 whose centre lies `away` units outside the sphere's surface, shuffled -> (positions, is_clump)"""
    from util import sphere_points
    rng = np.random.default_rng(seed)
    sizes = [32, 32, 32]
    pos, _ = sphere_points(rng, sizes, n, noise=0.05)
    centre, rad = (np.array(sizes) - 1) / 2.0, 0.3 * (min(sizes) - 1)
    d = rng.normal(size=(clump, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * (0.8 * rng.uniform(0, 1, (clump, 1)) ** (1.0 / 3.0))
    planted = centre + np.array([rad + away, 0.0, 0.0]) + d
    allp = np.concatenate([pos, planted.astype(np.float32)])
    flag = np.concatenate([np.zeros(n, bool), np.ones(clump, bool)])
    perm = rng.permutation(len(allp))
    return np.ascontiguousarray(allp[perm], np.float32), flag[perm]


def tie_cloud(b_first):
    """1-D, for eps = 1 and min_points = 4: the quadruples A = {-1, -1.5, -1.75, -2} and B = {1, 1.5, 1.75, 2}, every member
    core, 2 apart and so two clusters, and a point at 0 that reaches only -1 and 1, both at s = 1 exactly: not core, a border
    point with a tie.  The cluster numbers go one way (index 0 belongs to A with b_first, to B without) and the tie the other:
    index 1 is B's near point with b_first, A's without, index 3 the other one.  -> (positions (9, 1), the labels by hand)"""
    A, B = [-1.0, -1.5, -1.75, -2.0], [1.0, 1.5, 1.75, 2.0]
    near, far = (B, A) if b_first else (A, B)                # index 1 comes from `near`, index 0 from `far`
    x = [far[3], near[0], 0.0, far[0], far[1], far[2], near[1], near[2], near[3]]
    labels = [0, 1, 1, 0, 0, 0, 1, 1, 1]                      # the border point follows index 1, in cluster 1
    return np.float32(x).reshape(-1, 1), np.int32(labels)
