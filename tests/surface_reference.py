"""Numpy oracle of the surface-distance contract (include/fi_hip.h fi_surface_distance / fi_redistance): test
infrastructure only.  Every product, sum and quotient is a float32 operation on its own (one rounding each), in the
contract's order, as the device computes them with -ffp-contract=off:

  - dot products sum in ascending axes from the first term;
  - segment (a, b): ab = b - a; t = dot(q - a, ab) / dot(ab, ab) when dot(ab, ab) > 0, else 0; t clamped to [0, 1];
    c = a + t ab;
  - triangle (a, b, c): Ericson's ClosestPtPointTriangle (Real-Time Collision Detection 5.1.5), its Voronoi-region tests in
    its order and its expressions.  The branch taken dividing by a denominator that is not > 0 (the face's (va + vb) + vc,
    an edge region's d1 - d3, d2 - d6 or (d4 - d3) + (d5 - d6)) makes the triangle degenerate: the nearest of its three
    edges' segment points, ab, bc, ca, the first on ties;
  - c clamped per axis into the primitive's vertex box; s = 0 + (q_0 - c_0)^2 + ... in ascending axes;
  - best = min s over the usable primitives (every vertex coordinate finite), the smallest index reaching it, its c;
    sqrtf(best) > max_distance or nothing usable: +inf, -1, NaN point; a non-finite query: NaN, -1, NaN point.

The brute force evaluates, per chunk of queries, only the primitives whose box lower bound (formed like s) is within a
generous margin of an upper bound of the best s (the distance to each primitive's first vertex): every primitive that
can reach the minimum is among them (tests/test_surface_reference.py checks this against the unfiltered search).

Redistancing builds the mesh with tests/iso_reference.py (fi_iso_extract) or tests/dual_reference.py (fi_dual_contour),
both bit-equal to the device, and signs the distances by the producer's own inside rule.  Only numpy."""
import numpy as np

import dual_reference
import iso_reference
from nearest_reference import lattice_points

F = np.float32


class Unsupported(Exception):
    pass


class Invalid(Exception):
    pass


def _dot(u, v):
    s = u[0] * v[0]
    for d in range(1, len(u)):
        s = s + u[d] * v[d]
    return s


def _sq(q, c):
    s = np.zeros(q[0].shape, F)
    for d in range(len(q)):
        e = q[d] - c[d]
        s = s + e * e
    return s


def segment_points(q, a, b):
    """the segment rule before the box clamp; q, a, b: per-axis float32 arrays"""
    D = len(q)
    ab = [b[d] - a[d] for d in range(D)]
    aq = [q[d] - a[d] for d in range(D)]
    den = _dot(ab, ab)
    pos = den > 0
    with np.errstate(all="ignore"):
        t = np.where(pos, _dot(aq, ab) / np.where(pos, den, F(1)), F(0)).astype(F)
    t = np.where(t < 0, F(0), np.where(t > 1, F(1), t))
    return [a[d] + t * ab[d] for d in range(D)]


def _degenerate(q, a, b, c):
    p0, p1, p2 = segment_points(q, a, b), segment_points(q, b, c), segment_points(q, c, a)
    s0, s1, s2 = _sq(q, p0), _sq(q, p1), _sq(q, p2)
    take1 = s1 < s0
    best = np.where(take1, s1, s0)
    take2 = s2 < best
    return [np.where(take2, p2[d], np.where(take1, p1[d], p0[d])) for d in range(3)]


def triangle_points(p, a, b, c):
    """Ericson's closest point before the box clamp, with the degenerate rule; (points, region (0 A, 1 B, 2 AB, 3 C, 4 AC,
    5 BC, 6 face), degenerate flags)"""
    ab = [b[d] - a[d] for d in range(3)]
    ac = [c[d] - a[d] for d in range(3)]
    ap = [p[d] - a[d] for d in range(3)]
    bp = [p[d] - b[d] for d in range(3)]
    cp = [p[d] - c[d] for d in range(3)]
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    regions = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0),
               (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
    r = np.select(regions, [0, 1, 2, 3, 4, 5], 6)
    num = np.where(r == 2, d1, np.where(r == 4, d2, e43))
    den = np.where(r == 2, d1 - d3, np.where(r == 4, d2 - d6, e43 + e56))
    with np.errstate(all="ignore"):
        t = num / den
        tot = (va + vb) + vc
        inv = F(1) / tot
    v, w = vb * inv, vc * inv
    edge = (r == 2) | (r == 4) | (r == 5)
    degen = (edge & ~(den > 0)) | ((r == 6) & ~(tot > 0))
    out = []
    with np.errstate(all="ignore"):
        for d in range(3):
            direction = np.where(r == 2, ab[d], np.where(r == 4, ac[d], c[d] - b[d]))
            ep = np.where(r != 5, a[d], b[d]) + t * direction
            fp = (a[d] + ab[d] * v) + ac[d] * w
            out.append(np.select([r == 0, r == 1, r == 3, edge], [a[d], b[d], c[d], ep], fp).astype(F))
    if degen.any():
        k = np.flatnonzero(degen)
        alt = _degenerate([x[k] for x in p], [x[k] for x in a], [x[k] for x in b], [x[k] for x in c])
        for d in range(3):
            out[d][k] = alt[d]
    return out, r, degen


def primitive_points(q, verts):
    """(clamped closest points (per-axis arrays), s) of queries q against primitives verts = [vertex k][axis] arrays, pairwise"""
    D = len(q)
    with np.errstate(all="ignore"):
        if D == 3:
            c = triangle_points(q, *verts)[0]
        else:
            c = segment_points(q, *verts)
        lo = [verts[0][d] for d in range(D)]
        hi = [verts[0][d] for d in range(D)]
        for k in range(1, D):
            lo = [np.minimum(lo[d], verts[k][d]) for d in range(D)]
            hi = [np.maximum(hi[d], verts[k][d]) for d in range(D)]
        c = [np.where(c[d] < lo[d], lo[d], np.where(c[d] > hi[d], hi[d], c[d])).astype(F) for d in range(D)]
        return c, _sq(q, c)


def _mesh(vertices, indices, ndim):
    if ndim not in (2, 3):
        raise Unsupported("ndim %d" % ndim)
    V = np.ascontiguousarray(vertices, F).reshape(-1, ndim)
    I = np.ascontiguousarray(indices, np.int64).reshape(-1, ndim)
    if I.size and (I.min() < 0 or I.max() >= V.shape[0]):
        raise Invalid("index outside the vertices")
    P = V[I]                                                   # (np, vertex, axis)
    keep = np.flatnonzero(np.all(np.isfinite(P), axis=(1, 2)))
    return P[keep], keep


def _lb(Q, lo, hi):
    """(m, k) box lower bounds, formed like s"""
    s = np.zeros((Q.shape[0], lo.shape[0]), F)
    for d in range(Q.shape[1]):
        q = Q[:, d][:, None]
        g = np.where(q < lo[None, :, d], lo[None, :, d] - q, np.where(q > hi[None, :, d], q - hi[None, :, d], F(0)))
        s = s + g * g
    return s


def distance(vertices, indices, queries, ndim, max_distance=np.inf, filtered=True, chunk_pairs=1 << 22):
    """(distances float32 (m,), primitives int64 (m,), closest float32 (m, ndim)) for `queries` (x fastest)"""
    P, keep = _mesh(vertices, indices, ndim)
    Q = np.ascontiguousarray(queries, F).reshape(-1, ndim)
    m = Q.shape[0]
    md = F(max_distance)
    dist = np.full(m, np.inf, F)
    idx = np.full(m, -1, np.int64)
    closest = np.full((m, ndim), np.nan, F)
    qok = np.all(np.isfinite(Q), axis=1)
    dist[~qok] = np.nan
    rows = np.flatnonzero(qok)
    if P.shape[0] == 0 or rows.size == 0:
        return dist, idx, closest
    lo, hi = P.min(axis=1), P.max(axis=1)
    step = max(1, chunk_pairs // P.shape[0])
    for b0 in range(0, rows.size, step):
        r = rows[b0: b0 + step]
        if filtered:
            with np.errstate(over="ignore"):
                lb = _lb(Q[r], lo, hi)
                e = Q[r][:, None, :].astype(np.float64) - P[None, :, 0, :]
                ub = np.min(np.sum(e * e, axis=2), axis=1) * 1.001 + 0.01
            qi, pj = np.nonzero(lb <= ub[:, None])
        else:
            qi, pj = np.divmod(np.arange(r.size * P.shape[0]), P.shape[0])
        q = [Q[r[qi], d] for d in range(ndim)]
        verts = [[P[pj, k, d] for d in range(ndim)] for k in range(ndim)]
        c, s = primitive_points(q, verts)
        j = keep[pj]
        order = np.lexsort((j, s, qi))                          # NaN s sorts last within a query: never the best
        qs = qi[order]
        first = order[np.r_[True, qs[1:] != qs[:-1]]]
        good = ~np.isnan(s[first])
        first = first[good]
        out = r[qi[first]]
        with np.errstate(over="ignore"):
            d = np.sqrt(s[first]).astype(F)
        near = ~(d > md)
        first, out, d = first[near], out[near], d[near]
        dist[out] = d
        idx[out] = j[first]
        closest[out] = np.stack([c[k][first] for k in range(ndim)], axis=1)
    return dist, idx, closest


def distance_field(vertices, indices, sizes, max_distance=np.inf):
    return distance(vertices, indices, lattice_points(sizes), len(sizes), max_distance)[:2]


def surface(field, sizes, iso=0.0, method="iso"):
    """(vertices, indices, inside (N,) bool) of the producer's mesh and inside rule"""
    f = np.ascontiguousarray(field, F).reshape(-1)
    if method == "iso":
        v, _n, i, _k = iso_reference.extract(f, sizes, iso)
        inside = f < F(iso)
    elif method == "dual":
        v, _n, i, _k = dual_reference.contour(f, sizes, iso)[:4]
        inside = dual_reference.distances(f, iso) <= F(0)
    else:
        raise ValueError(method)
    return v, i, inside


def redistance(field, sizes, iso=0.0, method="iso", max_distance=np.inf, at=None):
    """(signed distances float32, primitives int64) of every lattice point (x fastest), or of the linear indices `at`"""
    sizes = [int(s) for s in sizes]
    if len(sizes) not in (2, 3):
        raise Unsupported("ndim %d" % len(sizes))
    v, i, inside = surface(field, sizes, iso, method)
    pts = lattice_points(sizes)
    if at is not None:
        at = np.asarray(at, np.int64)
        pts, inside = pts[at], inside[at]
    d, j, _c = distance(v, i, pts, len(sizes), max_distance)
    return np.where(inside, -d, d), j
