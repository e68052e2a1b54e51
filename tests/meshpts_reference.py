"""Numpy restatement of the contract of fi_mesh_sample / fi_mesh_deviation (include/fi_hip.h): points spread
over a mesh by area and the deviation of a mesh from a surface.  Test infrastructure, independent of the device code.  Every
floating-point step is written the way the contract states it -- fp64 from the fp32 coordinates, one rounding per operation;
integers are uint64 and wrap -- so that the arrays and figures returned are the bytes the device must produce.  Distances
come through tests/surface_reference.py (fi_surface_distance's own restatement).  Only numpy."""
import numpy as np

import surface_reference as SR

FACE, VERTEX = 0, 1
NORMALS = {"face": FACE, "vertex": VERTEX}
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
BLOCK = 256


class Invalid(Exception):
    """what the device answers with FI_ERR_INVALID"""


class Unsupported(Exception):
    """what the device answers with FI_ERR_UNSUPPORTED"""


def _rows(indices, D):
    return np.asarray(indices, np.int64).reshape(-1, D)


def bits_for(count):
    """key bits that tell `count` values apart (at least one)"""
    b = 1
    while (1 << b) < count:
        b += 1
    return b


def mix(z):
    """splitmix64's finaliser on uint64 arrays (wrapping)"""
    z = np.asarray(z, np.uint64).copy()
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def uniform(seed, counters):
    """u(c) = (mix(seed + (c + 1) golden) >> 11) 2^-53 -> float64 in [0, 1)"""
    c = np.asarray(counters, np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & (2 ** 64 - 1)) + (c + np.uint64(1)) * GOLDEN
        return (mix(z) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def face_normals(pos, idx):
    """(n_p float64 (P, D), its length w_p with the squares summed in axis order) from the fp32 positions"""
    p = np.asarray(pos, np.float32).astype(np.float64)
    a, b = p[idx[:, 0]], p[idx[:, 1]]
    with np.errstate(all="ignore"):
        if idx.shape[1] == 3:
            u, w = b - a, p[idx[:, 2]] - a
            n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                          u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
            return n, np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        e = b - a
        return np.stack([e[:, 1], -e[:, 0]], axis=1), np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])


def integer_weights(pos, idx):
    """(q uint64 (P,), C = its inclusive prefix sums, T) -- T == 0: nothing to sample"""
    P = len(idx)
    if P == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64), 0
    _n, w = face_normals(pos, idx)
    w = np.where(np.isfinite(w), w, 0.0)
    wmax = w.max()
    if not wmax > 0.0:
        q = np.zeros(P, np.uint64)
    else:
        k = min(32, 52 - bits_for(P))
        q = np.floor((w / wmax) * 2.0 ** k).astype(np.uint64)
    C = np.cumsum(q, dtype=np.uint64)
    return q, C, int(C[-1])


def strata(n, seed, T):
    """t of every sample: y = (((double)i + xi) / n) T; t = (uint64)y, T - 1 if t >= T"""
    i = np.arange(n, dtype=np.uint64)
    xi = uniform(seed, np.uint64(3) * i)
    y = i.astype(np.float64) + xi
    y = y / np.float64(n)
    y = y * np.float64(T)
    t = y.astype(np.uint64)
    return np.where(t >= np.uint64(T), np.uint64(T - 1), t)


def sample(vertices, normals, indices, n, seed=0, mode=FACE, want_normals=True):
    """-> (positions float32 (n, D), normals float32 (n, D) or None, primitives int64 (n,))"""
    pos = np.asarray(vertices, np.float32)
    D = pos.shape[1]
    idx = _rows(indices, D)
    if n < 0 or mode not in (FACE, VERTEX) or (want_normals and mode == VERTEX and normals is None):
        raise Invalid("arguments")
    if n >= 2 ** 31:
        raise Unsupported("n")
    if n == 0:
        return np.zeros((0, D), np.float32), (np.zeros((0, D), np.float32) if want_normals else None), np.zeros(0, np.int64)
    _q, C, T = integer_weights(pos, idx)
    if T == 0:
        raise Invalid("nothing to sample")
    t = strata(n, seed, T)
    prim = np.searchsorted(C, t, side="right").astype(np.int64)     # the number of entries of C that are <= t
    i3 = np.uint64(3) * np.arange(n, dtype=np.uint64)
    r1, r2 = uniform(seed, i3 + np.uint64(1)), uniform(seed, i3 + np.uint64(2))
    p64 = pos.astype(np.float64)
    tri = idx[prim]
    a, b = p64[tri[:, 0]], p64[tri[:, 1]]
    if D == 3:
        flip = r1 + r2 > 1.0
        r1, r2 = np.where(flip, 1.0 - r1, r1), np.where(flip, 1.0 - r2, r2)
        c = p64[tri[:, 2]]
        x = (a + r1[:, None] * (b - a)) + r2[:, None] * (c - a)
    else:
        x = a + r1[:, None] * (b - a)
    out_n = None
    if want_normals:
        fn, fl = face_normals(pos, tri)
        f = fn / fl[:, None]
        if mode == VERTEX:
            nv = np.asarray(normals, np.float32).astype(np.float64)
            if D == 3:
                w0 = (1.0 - r1) - r2
                m = (w0[:, None] * nv[tri[:, 0]] + r1[:, None] * nv[tri[:, 1]]) + r2[:, None] * nv[tri[:, 2]]
                l2 = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
            else:
                w0 = 1.0 - r1
                m = w0[:, None] * nv[tri[:, 0]] + r1[:, None] * nv[tri[:, 1]]
                l2 = m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]
            with np.errstate(all="ignore"):
                ln = np.sqrt(l2)
                good = (ln > 0.0) & np.isfinite(ln)
                f = np.where(good[:, None], m / ln[:, None], f)
        with np.errstate(over="ignore"):
            out_n = f.astype(np.float32)
    with np.errstate(over="ignore"):
        return x.astype(np.float32), out_n, prim


def tree_sum(values):
    """the fixed-order sum of float64 values: blocks of 256 by the tree s[t] += s[t + w], w = 128 .. 1 (the tail padded with
    0.0), then the block sums one after the other, ascending, from 0.0"""
    v = np.asarray(values, np.float64)
    nb = (len(v) + BLOCK - 1) // BLOCK
    s = np.zeros(nb * BLOCK, np.float64)
    s[:len(v)] = v
    s = s.reshape(nb, BLOCK)
    w = BLOCK // 2
    while w > 0:
        s[:, :w] = s[:, :w] + s[:, w:2 * w]
        w //= 2
    total = np.float64(0.0)
    for b in range(nb):
        total = total + s[b, 0]
    return total


def nothing():
    return {"queries": 0, "counted": 0, "beyond": 0, "invalid": 0, "at": -1, "max": 0.0, "mean": 0.0, "rms": 0.0,
            "where": np.zeros(3, np.float32)}


def statistics(d, queries):
    """the figures of one query list: d float32 (n,), queries float32 (n, D)"""
    d = np.asarray(d, np.float32)
    out = nothing()
    if len(d) == 0:
        return out
    counted = np.isfinite(d)
    out["queries"] = len(d)
    out["counted"] = int(counted.sum())
    out["invalid"] = int(np.isnan(d).sum())
    out["beyond"] = len(d) - out["counted"] - out["invalid"]
    x = np.where(counted, d, np.float32(0)).astype(np.float64)
    s1, s2 = tree_sum(x), tree_sum(x * x)
    if out["counted"]:
        top = d[counted].max()
        out["at"] = int(np.flatnonzero(counted & (d == top))[0])
        out["max"] = float(top)
        out["mean"] = float(s1 / np.float64(out["counted"]))
        out["rms"] = float(np.sqrt(s2 / np.float64(out["counted"])))
        out["where"][:queries.shape[1]] = queries[out["at"]]
    return out


def deviation(a_vertices, a_indices, b_vertices, b_indices, samples=0, seed=0, max_distance=np.inf):
    """-> (of_samples, of_vertices, vertex_distances float32 (a's vertex count,)): a's samples and used vertices against b"""
    pos = np.asarray(a_vertices, np.float32)
    D = pos.shape[1]
    idx = _rows(a_indices, D)
    md = np.float32(max_distance)
    bv = np.asarray(b_vertices, np.float32)
    if samples < 0 or not md >= 0 or bv.ndim != 2 or bv.shape[1] != D:     # (a surface of another dimension)
        raise Invalid("arguments")
    bi = _rows(b_indices, D)
    of_s = nothing()
    if samples > 0 and len(idx) and integer_weights(pos, idx)[2] > 0:
        pts = sample(pos, None, idx, samples, seed, FACE, False)[0]
        of_s = statistics(SR.distance(bv, bi, pts, D, md)[0], pts)
    used = np.zeros(len(pos), bool)
    used[idx.reshape(-1)] = True
    members = np.flatnonzero(used)
    vd = np.full(len(pos), np.nan, np.float32)
    of_v = nothing()
    if len(members):
        d = SR.distance(bv, bi, pos[members], D, md)[0]
        vd[members] = d
        of_v = statistics(d, pos[members])
    return of_s, of_v, vd
