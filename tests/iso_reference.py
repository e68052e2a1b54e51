"""Independent numpy / Python implementation of the iso-contour contract (include/fi_hip.h, fi_iso_extract; DESIGN.md
"Iso-contours and iso-surfaces"): test infrastructure only.  It walks each active cell's faces and chains their segments
into loops at run time; it does not read the device tables (field_interpolation_amd/csrc/fi_iso_tables.h).

Lattice arrays are flat, x fastest.  extract() returns (vertices, normals, indices, keys) like field_interpolation_amd.IsoMesh.
"""
import itertools

import numpy as np


class Unsupported(Exception):
    pass


class NonFinite(Exception):
    pass


def edge_number(ndim, axis, offs):
    """local edge 2^(ndim-1) * axis + j, j = o1 + 2 o2 over the offsets along the other axes in increasing axis order"""
    others = [d for d in range(ndim) if d != axis]
    return (1 << (ndim - 1)) * axis + sum(offs[d] << i for i, d in enumerate(others))


def edge_corner(ndim, e):
    """(axis, lower corner offsets) of local edge e"""
    axis = e >> (ndim - 1)
    j = e & ((1 << (ndim - 1)) - 1)
    offs = [0] * ndim
    for i, d in enumerate(d for d in range(ndim) if d != axis):
        offs[d] = (j >> i) & 1
    return axis, tuple(offs)


def _ring_segments(ring, inside, ndim):
    """Segments of one face.  `ring`: its corners counter-clockwise as seen from the side the inside must lie to the RIGHT
    of (3-D: from outside the cube; 2-D: the ring is walked clockwise, x right, y up).  A segment runs from the edge on
    which the walk enters a run of inside corners to the edge on which it leaves it: every inside corner of a face whose
    two inside corners are diagonal is cut off by its own segment."""
    k = len(ring)
    ins = [inside[c] for c in ring]
    if all(ins) or not any(ins):
        return []

    def edge(c0, c1):
        a = next(d for d in range(ndim) if c0[d] != c1[d])
        lo = tuple(min(c0[d], c1[d]) for d in range(ndim))
        return edge_number(ndim, a, lo)

    segs = []
    for i in range(k):
        if not ins[i] and ins[(i + 1) % k]:      # the walk enters a run at edge (i, i+1)
            j = (i + 1) % k
            while ins[(j + 1) % k]:
                j = (j + 1) % k
            segs.append((edge(ring[i], ring[(i + 1) % k]), edge(ring[j], ring[(j + 1) % k])))
    return segs


_LOOPS = {}


def cell_primitives(ndim, inside):
    """inside: {corner offsets: bool}.  2-D: segments (start edge, end edge) by start edge; 3-D: triangles (loops by their
    smallest edge, each fanned from it)."""
    sig = (ndim, tuple(sorted(inside.items())))
    if sig in _LOOPS:
        return _LOOPS[sig]
    if ndim == 2:
        ring = [(0, 0), (0, 1), (1, 1), (1, 0)]      # clockwise (x right, y up): inside on the left of every segment
        prims = sorted(_ring_segments(ring, inside, 2))
    else:
        segs = []
        for n in range(3):
            u, w = [d for d in range(3) if d != n]
            for s in (0, 1):
                # outward normal (2s - 1) e_n; (u, w) counter-clockwise about e_n when e_u x e_w = e_n
                pos_orient = (n == 1) ^ (s == 1)     # e_u x e_w = +e_n for n = 0, 2 (u < w), -e_n for n = 1
                quad = [(0, 0), (1, 0), (1, 1), (0, 1)] if pos_orient else [(0, 0), (0, 1), (1, 1), (1, 0)]
                ring = []
                for a, b in quad:
                    c = [0, 0, 0]
                    c[n], c[u], c[w] = s, a, b
                    ring.append(tuple(c))
                segs += _ring_segments(ring, inside, 3)
        nxt = {}
        for a, b in segs:
            assert a not in nxt, "two segments start on one edge"
            nxt[a] = b
        prims = []
        todo = set(nxt)
        while todo:
            v0 = min(todo)
            loop = [v0]
            while nxt[loop[-1]] != v0:
                loop.append(nxt[loop[-1]])
                assert len(loop) <= 12
            todo -= set(loop)
            prims += [(v0, loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    _LOOPS[sig] = prims
    return prims


def case_inside(ndim, case):
    return {c: bool((case >> sum(o << d for d, o in enumerate(c))) & 1) for c in itertools.product((0, 1), repeat=ndim)}


def _gradient(f, ndim):
    """central differences (one-sided at the border) in fp32; f indexed [z][y][x] (x last)"""
    g = []
    half = np.float32(0.5)
    for a in range(ndim):
        ax = ndim - 1 - a
        n = f.shape[ax]
        d = np.zeros_like(f)
        if n >= 2:
            sl = lambda i, j: tuple(slice(i, j) if k == ax else slice(None) for k in range(ndim))  # noqa: E731
            if n >= 3:
                d[sl(1, n - 1)] = (f[sl(2, n)] - f[sl(0, n - 2)]) * half
            d[sl(0, 1)] = f[sl(1, 2)] - f[sl(0, 1)]
            d[sl(n - 1, n)] = f[sl(n - 1, n)] - f[sl(n - 2, n - 1)]
        g.append(d)
    return g


def extract(field, sizes, iso=0.0):
    sizes = [int(s) for s in sizes]
    ndim = len(sizes)
    if ndim == 1:
        raise Unsupported("1-D")
    f = np.asarray(field, np.float32).reshape(sizes[::-1])
    if not np.all(np.isfinite(f)):
        raise NonFinite()
    empty = (np.zeros((0, ndim), np.float32), np.zeros((0, ndim), np.float32), np.zeros((0, ndim), np.int32),
             np.zeros(0, np.int64))
    if min(sizes) < 2:
        return empty
    iso = np.float32(iso)
    inside = f < iso
    grad = _gradient(f, ndim)
    lin = np.arange(f.size, dtype=np.int64).reshape(f.shape)
    keys, pos, nrm = [], [], []
    for a in range(ndim):
        ax = ndim - 1 - a
        lo = tuple(slice(0, -1) if k == ax else slice(None) for k in range(ndim))
        hi = tuple(slice(1, None) if k == ax else slice(None) for k in range(ndim))
        cross = inside[lo] != inside[hi]
        idx = lin[lo][cross]
        fp, fq = f[lo][cross], f[hi][cross]
        dp, dq = fp - iso, fq - iso
        t = dp / (dp - dq)
        coords = np.stack(np.unravel_index(idx, f.shape)[::-1], axis=1).astype(np.float32)  # (x, y[, z])
        coords[:, a] = coords[:, a] + t
        one = np.float32(1)
        nv = np.stack([(one - t) * grad[d][lo][cross] + t * grad[d][hi][cross] for d in range(ndim)], axis=1)
        l2 = nv[:, 0] * nv[:, 0]
        for d in range(1, ndim):
            l2 = l2 + nv[:, d] * nv[:, d]
        ln = np.sqrt(l2)
        nv = np.where(ln[:, None] > 0, nv / np.where(ln > 0, ln, 1)[:, None], np.float32(0)).astype(np.float32)
        keys.append(ndim * idx + a)
        pos.append(coords)
        nrm.append(nv)
    keys = np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    pos = np.concatenate(pos)[order]
    nrm = np.concatenate(nrm)[order]
    # active cells in ascending linear index
    cells = np.ones(tuple(n - 1 for n in sizes[::-1]), bool)
    corner_in = []
    for c in itertools.product((0, 1), repeat=ndim):
        sl = tuple(slice(c[ndim - 1 - k], c[ndim - 1 - k] + n - 1) for k, n in enumerate(sizes[::-1]))
        corner_in.append((c, inside[sl]))
    anyin = np.zeros(cells.shape, bool)
    allin = np.ones(cells.shape, bool)
    case = np.zeros(cells.shape, np.int32)
    for c, m in corner_in:
        anyin |= m
        allin &= m
        case |= m.astype(np.int32) << sum(o << d for d, o in enumerate(c))
    act = anyin & ~allin
    cell_lin = lin[tuple(slice(0, n - 1) for n in sizes[::-1])][act]
    cell_case = case[act]
    order = np.argsort(cell_lin, kind="stable")
    prims = []
    strides = [int(np.prod(sizes[:d])) for d in range(ndim)]
    for li, cs in zip(cell_lin[order], cell_case[order]):
        for prim in cell_primitives(ndim, case_inside(ndim, int(cs))):
            row = []
            for e in prim:
                a, offs = edge_corner(ndim, e)
                p = int(li) + sum(o * s for o, s in zip(offs, strides))
                row.append(ndim * p + a)
            prims.append(row)
    if not prims:
        return (pos, nrm, np.zeros((0, ndim), np.int32), keys)
    idx = np.searchsorted(keys, np.asarray(prims, np.int64)).astype(np.int32)
    return pos, nrm, idx, keys


# ---- mesh checks ------------------------------------------------------------------------------------------------------------

def directed_edges(indices):
    """3-D: the directed edges of the triangles; 2-D: the segments themselves"""
    indices = np.asarray(indices)
    if indices.shape[1] == 2:
        return [tuple(r) for r in indices]
    return [(int(t[i]), int(t[(i + 1) % 3])) for t in indices for i in range(3)]


def watertight_oriented(indices):
    """every undirected edge used exactly twice, once in each direction (3-D); every vertex starts one segment and ends one
    (2-D)"""
    indices = np.asarray(indices)
    if indices.shape[1] == 2:
        s, e = np.bincount(indices[:, 0]), np.bincount(indices[:, 1])
        n = max(len(s), len(e))
        s, e = np.pad(s, (0, n - len(s))), np.pad(e, (0, n - len(e)))
        used = (s + e) > 0
        return bool(np.all(s[used] == 1) and np.all(e[used] == 1))
    d = directed_edges(indices)
    ds = set(d)
    return len(ds) == len(d) and all((b, a) in ds for a, b in d)


def signed_measure(vertices, indices):
    """2-D: signed area (inside on the left: positive); 3-D: signed volume (outward triangles: positive)"""
    v = np.asarray(vertices, np.float64)
    i = np.asarray(indices)
    if i.shape[1] == 2:
        a, b = v[i[:, 0]], v[i[:, 1]]
        return 0.5 * float(np.sum(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]))
    a, b, c = v[i[:, 0]], v[i[:, 1]], v[i[:, 2]]
    return float(np.sum(np.einsum("ij,ij->i", a, np.cross(b, c)))) / 6.0


def euler_characteristic(nv, indices):
    tri = np.asarray(indices)
    edges = {tuple(sorted(e)) for e in directed_edges(tri)}
    return int(nv) - len(edges) + len(tri)


def components(nv, indices):
    parent = list(range(nv))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for t in np.asarray(indices):
        for k in range(1, len(t)):
            ra, rb = find(int(t[0])), find(int(t[k]))
            if ra != rb:
                parent[ra] = rb
    return len({find(i) for i in range(nv)})
