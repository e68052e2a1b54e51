"""Numpy restatement of the ray contract (include/fi_hip.h fi_surface_raycast): test infrastructure only.
Every fp32 operation is a float32 operation on its own (one rounding each), every fp64 one a float64 operation, in the
order written here, as the device computes them with -ffp-contract=off.

A ray o + t d, t_min <= t <= t_max (closed), d not normalised.  A ray with a non-finite o or d, or d = 0: t = NaN,
primitive -1, NaN barycentrics, count 0.  Usable primitives: every vertex coordinate finite.

3-D (Woop, Benthin, Wald: Watertight Ray/Triangle Intersection, JCGT 2013):
  - kz = the axis of the largest |d| (the lowest on ties), kx, ky the next two in cyclic order, swapped when d[kz] < 0;
    Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz] in fp32;
  - per vertex in fp32: p = v - o, X = p[kx] - Sx p[kz], Y = p[ky] - Sy p[kz], Z = Sz p[kz];
  - in fp64 from the fp32 X, Y: U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax (exact products: exact signs and
    zeros); a candidate has U, V, W all >= 0 ("positive") or all <= 0, and not all zero;
  - a zero edge function is the triangle's only if it owns the edge: B->C belongs to U, C->A to V, A->B to W, with
    (dx, dy) = end - start, negated when the triangle is not positive; owned when dy > 0, or dy = 0 and dx < 0;
  - t = fp32(((U Az + V Bz) + W Cz) / ((U + V) + W)) (fp64), then t < min Z: min Z, t > max Z: max Z (fp32 min / max of the
    three Z); a hit when t_min <= t <= t_max; barycentrics fp32(V / det), fp32(W / det).
2-D: kz as above, kx the other axis; X = p[kx] - Sx p[kz], Z = Sz p[kz] in fp32; a segment (a, b) is crossed when
(Xa > 0) != (Xb > 0); in fp64 s = Xa / (Xa - Xb), t = fp32(Za + s (Zb - Za)), clamped into [min Z, max Z]; barycentric
fp32(s).

Closest hit: the smallest t in range, the smallest primitive index on ties; none: +inf, -1, NaN barycentrics.  Count: the
hits in range, saturated at limit.

Two modes.  Brute force tests every ray against every usable primitive.  The tree-filtered mode sorts the primitives by
a Morton code of their box centres into leaves of 8 under a balanced binary tree of boxes and tests a primitive only if
no box above it is pruned by the contract's rule: with the box corner chosen by the sign of Sx (Sy, Sz), the same fp32
expressions give Xmin, Xmax (Ymin, Ymax, Zmin, Zmax) of the box, and the box is pruned when Xmin > 0, Xmax < 0 (the same
in Y), Zmax < t_min or Zmin > t_max.  Rounding is monotone, so the bounds hold bit for bit and both modes must agree
bit for bit (tests/test_ray_reference.py).  Only numpy."""
import numpy as np

import surface_reference
from nearest_reference import lattice_points
from surface_reference import Invalid, Unsupported, _mesh  # noqa: F401

F = np.float32
D64 = np.float64
LEAF = 8
INT_MAX = 2**31 - 1


def _check_window(t_min, t_max):
    t_min, t_max = F(t_min), F(t_max)
    if np.isnan(t_min) or np.isnan(t_max) or t_min > t_max:
        raise Invalid("t_min %r, t_max %r" % (t_min, t_max))
    return t_min, t_max


class _Rays:
    """the usable rays of a call: rows (into the input), o (m, D), the permutation kx, ky, kz and the shear Sx, Sy, Sz"""

    def __init__(self, origins, directions, ndim):
        O = np.ascontiguousarray(origins, F).reshape(-1, ndim)
        Dr = np.ascontiguousarray(directions, F).reshape(-1, ndim)
        if Dr.shape[0] == 1 and O.shape[0] != 1:
            Dr = np.broadcast_to(Dr, O.shape)
        assert O.shape == Dr.shape
        self.n, self.ndim = O.shape[0], ndim
        ok = np.all(np.isfinite(O), axis=1) & np.all(np.isfinite(Dr), axis=1) & np.any(Dr != 0, axis=1)
        self.rows = np.flatnonzero(ok)
        self.take(O[self.rows], Dr[self.rows])

    def take(self, o, d):
        m = o.shape[0]
        r = np.arange(m)
        self.o = o
        kz = np.argmax(np.abs(d), axis=1) if m else np.zeros(0, np.int64)     # (the first maximum: the lowest axis)
        if self.ndim == 3:
            kx, ky = (kz + 1) % 3, (kz + 2) % 3
            neg = d[r, kz] < 0
            kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
        else:
            kx, ky = 1 - kz, None
        self.kx, self.ky, self.kz = kx, ky, kz
        with np.errstate(all="ignore"):
            dz = d[r, kz]
            self.Sx = d[r, kx] / dz
            self.Sy = d[r, ky] / dz if self.ndim == 3 else None
            self.Sz = F(1) / dz

    def chunk(self, b, e):
        c = object.__new__(_Rays)
        c.ndim = self.ndim
        c.o, c.kx, c.kz, c.Sx, c.Sz = self.o[b:e], self.kx[b:e], self.kz[b:e], self.Sx[b:e], self.Sz[b:e]
        c.ky = self.ky[b:e] if self.ndim == 3 else None
        c.Sy = self.Sy[b:e] if self.ndim == 3 else None
        return c


def _project(R, qi, v):
    """X, Y, Z (fp32) of the vertices v (pairs, D) seen from the rays qi"""
    o = R.o[qi]
    r = np.arange(qi.size)
    kx, kz = R.kx[qi], R.kz[qi]
    with np.errstate(all="ignore"):
        pz = v[r, kz] - o[r, kz]
        X = (v[r, kx] - o[r, kx]) - R.Sx[qi] * pz
        Y = None
        if R.ndim == 3:
            ky = R.ky[qi]
            Y = (v[r, ky] - o[r, ky]) - R.Sy[qi] * pz
        Z = R.Sz[qi] * pz
    return X, Y, Z


def _clamp(t, Zs):
    lo, hi = Zs[0], Zs[0]
    for z in Zs[1:]:
        lo, hi = np.minimum(lo, z), np.maximum(hi, z)
    return np.where(t < lo, lo, np.where(t > hi, hi, t)).astype(F)


def _pairs(R, qi, prims, t_min, t_max):
    """(hit flags, t fp32, barycentrics (pairs, D - 1) fp32) of the rays qi against the primitives prims (pairs, D, D)"""
    with np.errstate(all="ignore"):
        if R.ndim == 2:
            Xa, _y, Za = _project(R, qi, prims[:, 0])
            Xb, _y, Zb = _project(R, qi, prims[:, 1])
            hit = (Xa > 0) != (Xb > 0)
            xa, xb, za, zb = Xa.astype(D64), Xb.astype(D64), Za.astype(D64), Zb.astype(D64)
            s = xa / (xa - xb)
            t = _clamp((za + s * (zb - za)).astype(F), [Za, Zb])
            bary = s.astype(F)[:, None]
        else:
            Ax, Ay, Az = _project(R, qi, prims[:, 0])
            Bx, By, Bz = _project(R, qi, prims[:, 1])
            Cx, Cy, Cz = _project(R, qi, prims[:, 2])
            ax, ay, bx, by, cx, cy = [a.astype(D64) for a in (Ax, Ay, Bx, By, Cx, Cy)]
            U = cx * by - cy * bx
            V = ax * cy - ay * cx
            W = bx * ay - by * ax
            pos = (U >= 0) & (V >= 0) & (W >= 0)
            neg = (U <= 0) & (V <= 0) & (W <= 0)
            hit = (pos | neg) & ~((U == 0) & (V == 0) & (W == 0))

            def owns(x0, y0, x1, y1):
                up = (y1 > y0) | ((y1 == y0) & (x1 < x0))
                down = (y1 < y0) | ((y1 == y0) & (x1 > x0))
                return np.where(pos, up, down)
            hit &= (U != 0) | owns(Bx, By, Cx, Cy)
            hit &= (V != 0) | owns(Cx, Cy, Ax, Ay)
            hit &= (W != 0) | owns(Ax, Ay, Bx, By)
            det = (U + V) + W
            num = (U * Az.astype(D64) + V * Bz.astype(D64)) + W * Cz.astype(D64)
            t = _clamp((num / det).astype(F), [Az, Bz, Cz])
            bary = np.stack([(V / det).astype(F), (W / det).astype(F)], axis=1)
        hit = hit & (t >= t_min) & (t <= t_max)
    return hit, t, bary


def _morton(P):
    c = 0.5 * (P.min(axis=1).astype(D64) + P.max(axis=1))
    lo, ext = c.min(axis=0), np.ptp(c, axis=0)
    q = np.where(ext > 0, (c - lo) / np.where(ext > 0, ext, 1) * 1023, 0).astype(np.int64)
    key = np.zeros(P.shape[0], np.int64)
    for b in range(10):
        for d in range(P.shape[2]):
            key |= ((q[:, d] >> b) & 1) << (b * P.shape[2] + d)
    return np.argsort(key, kind="stable")


class Tree:
    """leaves of LEAF primitives in Morton order under a balanced binary tree of boxes: levels[0] the root ... levels[-1]
    the leaves, each (lo, hi) of (nodes, D); an empty node has lo = +inf > hi = -inf"""

    def __init__(self, P):
        self.order = _morton(P)
        S = P[self.order]
        nf, D = S.shape[0], S.shape[2]
        leaves = (nf + LEAF - 1) // LEAF
        H = 0
        while (1 << H) < leaves:
            H += 1
        lo = np.full((1 << H, D), np.inf, F)
        hi = np.full((1 << H, D), -np.inf, F)
        for j in range(leaves):
            s = S[j * LEAF: (j + 1) * LEAF].reshape(-1, D)
            lo[j], hi[j] = s.min(axis=0), s.max(axis=0)
        self.levels = [(lo, hi)]
        while lo.shape[0] > 1:
            lo = np.minimum(lo[0::2], lo[1::2])
            hi = np.maximum(hi[0::2], hi[1::2])
            self.levels.insert(0, (lo, hi))
        self.nf = nf


def admit(R, lo, hi, t_min, t_max):
    """(rays, nodes) flags: the contract's rule does not prune the box"""
    r = np.arange(R.o.shape[0])

    def rel(B, k):
        return B.T[k] - R.o[r, k][:, None]
    with np.errstate(all="ignore"):
        lz, hz = rel(lo, R.kz), rel(hi, R.kz)
        prune = np.zeros(lz.shape, bool)
        for k, S in ((R.kx, R.Sx), (R.ky, R.Sy)):
            if k is None:
                continue
            up = (S >= 0)[:, None]
            mn = rel(lo, k) - S[:, None] * np.where(up, hz, lz)
            mx = rel(hi, k) - S[:, None] * np.where(up, lz, hz)
            prune |= (mn > 0) | (mx < 0)
        zp = (R.Sz > 0)[:, None]
        zmin = R.Sz[:, None] * np.where(zp, lz, hz)
        zmax = R.Sz[:, None] * np.where(zp, hz, lz)
        prune |= (zmax < t_min) | (zmin > t_max)
    return ~prune & (lo[:, 0] <= hi[:, 0])[None, :]


def _candidates(R, P, tree, t_min, t_max, chunk_pairs):
    """chunks of (ray numbers qi, primitive rows pj into P) to test"""
    m, nf = R.o.shape[0], P.shape[0]
    if tree is None:
        step = max(1, chunk_pairs // nf)
        for b in range(0, m, step):
            e = min(m, b + step)
            qi, pj = np.divmod(np.arange((e - b) * nf), nf)
            yield qi + b, pj
        return
    step = max(1, chunk_pairs // (2 * tree.levels[-1][0].shape[0]))
    for b in range(0, m, step):
        e = min(m, b + step)
        Rc = R.chunk(b, e)
        ok = None
        for lo, hi in tree.levels:
            a = admit(Rc, lo, hi, t_min, t_max)
            ok = a if ok is None else (a & np.repeat(ok, 2, axis=1))
        qi, leaf = np.nonzero(ok)
        qi = np.repeat(qi, LEAF)
        slot = (leaf[:, None] * LEAF + np.arange(LEAF)[None, :]).reshape(-1)
        keep = slot < tree.nf
        yield qi[keep] + b, tree.order[slot[keep]]


def _hits(vertices, indices, ndim, origins, directions, t_min, t_max, filtered, chunk_pairs=1 << 21):
    """every hit of the call: (n rays, ray rows (hits,), t, primitive indices, barycentrics)"""
    t_min, t_max = _check_window(t_min, t_max)
    P, keep = _mesh(vertices, indices, ndim)
    R = _Rays(origins, directions, ndim)
    out = [np.zeros(0, np.int64), np.zeros(0, F), np.zeros(0, np.int64), np.zeros((0, ndim - 1), F)]
    if P.shape[0] and R.rows.size:
        tree = Tree(P) if filtered else None
        parts = []
        for qi, pj in _candidates(R, P, tree, t_min, t_max, chunk_pairs):
            hit, t, bary = _pairs(R, qi, P[pj], t_min, t_max)
            parts.append((R.rows[qi[hit]], t[hit], keep[pj[hit]], bary[hit]))
        out = [np.concatenate([p[k] for p in parts]) for k in range(4)]
    return R, out


def _closest(R, rows, t, j, bary, ndim):
    T = np.full(R.n, np.nan, F)
    T[R.rows] = np.inf
    prim = np.full(R.n, -1, np.int64)
    B = np.full((R.n, ndim - 1), np.nan, F)
    if rows.size:
        order = np.lexsort((j, t, rows))
        rs = rows[order]
        first = order[np.r_[True, rs[1:] != rs[:-1]]]
        T[rows[first]], prim[rows[first]], B[rows[first]] = t[first], j[first], bary[first]
    return T, prim, B


def raycast(vertices, indices, ndim, origins, directions, t_min=0.0, t_max=np.inf, filtered=True):
    """(t float32 (n,), primitives int64 (n,), barycentrics float32 (n, ndim - 1)) of the closest hits"""
    R, (rows, t, j, bary) = _hits(vertices, indices, ndim, origins, directions, t_min, t_max, filtered)
    return _closest(R, rows, t, j, bary, ndim)


def cast_and_count(vertices, indices, ndim, origins, directions, t_min=0.0, t_max=np.inf, filtered=True):
    """raycast's three results and count_hits' unsaturated counts from one pass over the hits"""
    R, (rows, t, j, bary) = _hits(vertices, indices, ndim, origins, directions, t_min, t_max, filtered)
    return _closest(R, rows, t, j, bary, ndim) + (np.bincount(rows, minlength=R.n).astype(np.int32),)


def count_hits(vertices, indices, ndim, origins, directions, t_min=0.0, t_max=np.inf, limit=INT_MAX, filtered=True):
    """counts int32 (n,) of the hits in range, saturated at limit"""
    if limit < 1:
        raise Invalid("limit %d" % limit)
    R, (rows, _t, _j, _b) = _hits(vertices, indices, ndim, origins, directions, t_min, t_max, filtered)
    return np.minimum(np.bincount(rows, minlength=R.n), limit).astype(np.int32)


def contains(vertices, indices, ndim, points, direction=None, filtered=True):
    """bool (n,): the parity of the crossings of the ray from each point along `direction` (+x), t in [0, +inf)"""
    d = np.zeros((1, ndim), F)
    d[0, 0] = 1
    if direction is not None:
        d[0] = np.asarray(direction, F)
    c = count_hits(vertices, indices, ndim, points, d, 0.0, np.inf, INT_MAX, filtered)
    return (c & 1).astype(bool)


def signed_distance(vertices, indices, ndim, queries, max_distance=np.inf):
    """surface_reference.distance with the distances negated where contains() holds along +x"""
    d, j, c = surface_reference.distance(vertices, indices, queries, ndim, max_distance)
    inside = contains(vertices, indices, ndim, queries)
    return np.where(inside, -d, d), j, c


def signed_distance_field(vertices, indices, sizes, max_distance=np.inf):
    return signed_distance(vertices, indices, len(sizes), lattice_points(sizes), max_distance)[:2]
