"""Numpy restatement of the point-cloud cleaning contract (include/fi_hip.h fi_radius_count .. fi_cloud_thin; DESIGN.md
4.19): the definition the device is held to bit for bit.  Brute force over every pair with nearest_reference.sq_dist's fp32
arithmetic, a stable argsort for the tie rule, fp64 sums written one operation at a time (elementwise numpy operations round
like the scalar ones) and meshpts_reference.tree_sum for the fixed-order sum.  It shares nothing with the device path: no
tree, no Morton order, no list.  Only numpy."""
import numpy as np

import nearest_reference as NR
import normals_reference as N
from meshpts_reference import tree_sum

MEAN, FIRST = "mean", "first"
CELL_BIAS = 1 << 20


def _finite(P):
    return np.all(np.isfinite(P), axis=1)


def _chunks(rows, per_row, chunk_pairs=1 << 22):
    step = max(1, chunk_pairs // max(1, per_row))
    for b in range(0, rows.size, step):
        yield rows[b: b + step]


def radius_count(points, queries, ndim, radius, limit=np.iinfo(np.int32).max):
    """counts int32 (m,): min(limit, the finite points with sqrtf(s) <= radius), -1 for a non-finite query"""
    P, Q = NR._as_points(points, ndim), NR._as_points(queries, ndim)
    r32 = np.float32(radius)
    Pf = P[_finite(P)]
    counts = np.zeros(Q.shape[0], np.int64)
    qok = _finite(Q)
    counts[~qok] = -1
    if Pf.shape[0] > 0:
        with np.errstate(over="ignore"):
            for r in _chunks(np.flatnonzero(qok), Pf.shape[0]):
                counts[r] = np.minimum(limit, (np.sqrt(NR.sq_dist(Pf, Q[r])) <= r32).sum(axis=1))
    return counts.astype(np.int32)


def neighbour_table(points, ndim, kmax=N.MAX_K):
    """(the finite points' indices (nf,), d float32 (nf, min(kmax, nf - 1))): sqrtf(s) of every finite point's nearest OTHER
    finite points in the order of the pairs (s, j) -- what neighbour_distances takes its first k from, for any k <= kmax"""
    P = NR._as_points(points, ndim)
    keep = np.flatnonzero(_finite(P))                         # ascending: a stable sort keeps the smallest index first
    Pf = P[keep]
    nf = Pf.shape[0]
    have = max(0, min(kmax, nf - 1))
    d = np.zeros((nf, have), np.float32)
    if have > 0:
        with np.errstate(over="ignore"):
            for r in _chunks(np.arange(nf), nf):
                s = NR.sq_dist(Pf, Pf[r])
                order = np.argsort(s, axis=1, kind="stable")
                order = order[order != r[:, None]].reshape(r.size, nf - 1)[:, :have]      # the point itself leaves by its index
                d[r] = np.sqrt(np.take_along_axis(s, order, axis=1))
    return keep, d


def neighbour_distances(points, ndim, k, max_distance=np.inf, table=None):
    """(mean float32 (n,), kth float32 (n,), counts int32 (n,)) of every point over its k nearest OTHER points; table: a
    neighbour_table(points, ndim, kmax >= k) made earlier"""
    if not 1 <= k <= N.MAX_K:
        raise ValueError("k must be 1..%d" % N.MAX_K)
    n = NR._as_points(points, ndim).shape[0]
    keep, d = table if table is not None else neighbour_table(points, ndim, k)
    d = d[:, :k]
    md = np.float32(max_distance)
    mean = np.full(n, np.nan, np.float32)
    kth = np.full(n, np.nan, np.float32)
    counts = np.zeros(n, np.int32)
    ok = d <= md                                              # (a prefix of every row: d ascends)
    m = ok.sum(axis=1)
    acc = np.zeros(keep.size, np.float64)
    for c in range(d.shape[1]):                               # the sum from 0.0 in result order
        acc = acc + np.where(ok[:, c], d[:, c].astype(np.float64), 0.0)
    got = m > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean[keep] = np.where(got, (acc / m).astype(np.float32), np.float32(np.inf))
    last = d[np.arange(keep.size), np.maximum(m, 1) - 1] if d.shape[1] else np.zeros(keep.size, np.float32)
    kth[keep] = np.where(got, last, np.float32(np.inf))
    counts[keep] = m
    return mean, kth, counts


def statistics(mean, std_ratio):
    """(keep uint8 (n,), stats) of the statistical rule over neighbour_distances' mean"""
    x = np.asarray(mean, np.float32).astype(np.float64)
    counted = np.isfinite(x)
    cnt = int(counted.sum())
    stats = {"counted": cnt, "kept": 0, "mean": 0.0, "stddev": 0.0, "threshold": 0.0}
    if cnt == 0:
        return np.zeros(x.size, np.uint8), stats
    with np.errstate(invalid="ignore", over="ignore"):
        mu = tree_sum(np.where(counted, x, 0.0)) / np.float64(cnt)
        e = x - mu
        sigma = np.sqrt(tree_sum(np.where(counted, e * e, 0.0)) / np.float64(cnt))
        t = mu + np.float64(np.float32(std_ratio)) * sigma
        keep = counted & (x <= t)
    stats.update(kept=int(keep.sum()), mean=float(mu), stddev=float(sigma), threshold=float(t))
    return keep.astype(np.uint8), stats


def statistical_outliers(points, ndim, k, std_ratio, max_distance=np.inf):
    return statistics(neighbour_distances(points, ndim, k, max_distance)[0], std_ratio)


def radius_outliers(points, ndim, radius, min_neighbours):
    """keep uint8 (n,): finite, and min_neighbours finite points other than itself within the radius"""
    P = NR._as_points(points, ndim)
    r32 = np.float32(radius)
    idx = np.flatnonzero(_finite(P))
    Pf = P[idx]
    keep = np.zeros(P.shape[0], np.uint8)
    with np.errstate(over="ignore"):
        for r in _chunks(np.arange(Pf.shape[0]), Pf.shape[0]):
            within = np.sqrt(NR.sq_dist(Pf, Pf[r])) <= r32
            within[np.arange(r.size), r] = False              # the point itself, by its index
            keep[idx[r]] = within.sum(axis=1) >= min_neighbours
    return keep


def thin(positions, ndim, cell, origin=None, mode=MEAN, normals=None, values=None):
    """the occupied cells in ascending key order -> dict: positions, normals, values (None where none came in), counts int32,
    indices int64, cell_map int32 (n,)"""
    P = NR._as_points(positions, ndim)
    n = P.shape[0]
    o = np.zeros(ndim, np.float32) if origin is None else np.asarray(origin, np.float32).reshape(ndim)
    Nm = None if normals is None else NR._as_points(normals, ndim)
    V = None if values is None else np.ascontiguousarray(values, np.float32).reshape(n)
    fin = np.flatnonzero(_finite(P))
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.floor((P[fin] - o) / np.float32(cell))          # fp32 throughout
    if not np.all(np.abs(c) < np.float32(CELL_BIAS)):
        raise ValueError("a point lies 2^20 cells or more from the origin")
    key = np.zeros(fin.size, np.int64)
    for a in range(ndim):
        key |= (c[:, a].astype(np.int64) + CELL_BIAS) << (21 * a)
    _, number = np.unique(key, return_inverse=True)
    nc = int(number.max()) + 1 if fin.size else 0
    cell_map = np.full(n, -1, np.int32)
    cell_map[fin] = number
    order = fin[np.argsort(number, kind="stable")]             # by cell, ascending index within one
    counts = np.bincount(number, minlength=nc).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(counts)])[:nc]
    lowest = order[start]
    out = {"counts": counts.astype(np.int32), "indices": lowest.astype(np.int64), "cell_map": cell_map, "normals": None,
           "values": None}
    if mode == FIRST:
        out["positions"] = P[lowest]
        if Nm is not None:
            out["normals"] = Nm[lowest]
        if V is not None:
            out["values"] = V[lowest]
        return out
    sx = np.zeros((nc, ndim), np.float64)
    sn = np.zeros((nc, ndim), np.float64)
    sv = np.zeros(nc, np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for r in range(int(counts.max()) if nc else 0):       # every cell's r-th member, the sums one after the other
            cells = np.flatnonzero(counts > r)
            member = order[start[cells] + r]
            sx[cells] = sx[cells] + P[member].astype(np.float64)
            if Nm is not None:
                sn[cells] = sn[cells] + Nm[member].astype(np.float64)
            if V is not None:
                sv[cells] = sv[cells] + V[member].astype(np.float64)
        m = counts.astype(np.float64)
        out["positions"] = (sx / m[:, None]).astype(np.float32)
        if V is not None:
            out["values"] = (sv / m).astype(np.float32)
        if Nm is not None:
            l2 = sn[:, 0] * sn[:, 0]
            for a in range(1, ndim):
                l2 = l2 + sn[:, a] * sn[:, a]
            length = np.sqrt(l2)
            out["normals"] = np.where((length > 0.0)[:, None], (sn / length[:, None]).astype(np.float32), np.float32(0.0))
    return out


def clean(positions, ndim, normals=None, values=None, cell=None, k=None, std_ratio=2.0, radius=None, min_neighbours=2,
          max_distance=np.inf):
    """thin, radius filter, statistical filter, whichever are asked for, in that order -> (positions, normals, values, report)"""
    pos = NR._as_points(positions, ndim)
    nrm = None if normals is None else NR._as_points(normals, ndim)
    val = None if values is None else np.ascontiguousarray(values, np.float32)
    report = {"input": len(pos)}
    if cell is not None:
        t = thin(pos, ndim, cell, normals=nrm, values=val)
        report["thinned"] = len(pos) - len(t["positions"])
        pos, nrm, val = t["positions"], t["normals"], t["values"]
    if radius is not None:
        keep = radius_outliers(pos, ndim, radius, min_neighbours).astype(bool)
        report["radius"] = int((~keep).sum())
        pos, nrm, val = (a if a is None else a[keep] for a in (pos, nrm, val))
    if k is not None:
        keep, stats = statistical_outliers(pos, ndim, k, std_ratio, max_distance)
        keep = keep.astype(bool)
        report["statistical"] = int((~keep).sum())
        report["stats"] = stats
        pos, nrm, val = (a if a is None else a[keep] for a in (pos, nrm, val))
    report["output"] = len(pos)
    return pos, nrm, val, report


def planted_cloud(seed, n=4000, planted=36):
    """the sphere scan of the tests with stray returns planted: util.sphere_points(rng, [32, 32, 32], n, noise=0.05) plus
    `planted` points uniform in [-4, 35]^3 at least 2 units from the sphere surface, shuffled -> (positions, is_planted)"""
    from util import sphere_points
    rng = np.random.default_rng(seed)
    sizes = [32, 32, 32]
    pos, _ = sphere_points(rng, sizes, n, noise=0.05)
    centre, rad = (np.array(sizes) - 1) / 2.0, 0.3 * (min(sizes) - 1)
    stray = []
    while len(stray) < planted:
        p = rng.uniform(-4.0, 35.0, 3)
        if abs(np.linalg.norm(p - centre) - rad) >= 2.0:
            stray.append(p)
    allp = np.concatenate([pos, np.array(stray, np.float32)])
    flag = np.concatenate([np.zeros(n, bool), np.ones(planted, bool)])
    perm = rng.permutation(len(allp))
    return np.ascontiguousarray(allp[perm], np.float32), flag[perm]
