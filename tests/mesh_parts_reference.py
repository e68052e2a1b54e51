"""Numpy restatement of the mesh-parts contract (include/fi_hip.h fi_mesh_create .. fi_mesh_select): test
infrastructure, independent of the device code.  Labels, counts, bounding boxes and the selected sub-mesh are exact; the
measures come as per-primitive fp64 terms (and the magnitudes M of the error bound) that the caller sums with math.fsum.

Also the fields the CPU and the GPU tests share (fixture_3d, fixture_2d, checkerboard)."""
import math

import numpy as np


# ---- parts --------------------------------------------------------------------------------------------------------------

def _rows(indices, dtype=np.int64):
    """indices as (P, vertices per primitive); an empty list keeps the width of its shape (3 where it has none)"""
    a = np.asarray(indices, dtype)
    if a.size == 0:
        return a.reshape(0, a.shape[1] if a.ndim == 2 and a.shape[1] else 3)
    return a.reshape(len(a), -1)


def labels(nv, indices):
    """-> (C, vertex_labels int32 (-1: unused), primitive_labels int32).  Two primitives belong to one part when a chain of
    primitives joins them through shared vertex indices; parts are numbered by their smallest vertex, ascending."""
    idx = _rows(indices)
    parent = np.arange(nv, dtype=np.int64)
    a = np.repeat(idx[:, :1], idx.shape[1] - 1, axis=1).reshape(-1) if len(idx) else np.empty(0, np.int64)
    b = idx[:, 1:].reshape(-1) if len(idx) else np.empty(0, np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        differ = ra != rb
        if not differ.any():
            break
        hi, lo = np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ]
        np.minimum.at(parent, hi, lo)             # every root under the smallest root it touches: parents only fall
        while True:                               # ... and every vertex straight under its root again
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    used = np.zeros(nv, bool)
    used[idx.reshape(-1)] = True
    roots = np.flatnonzero(used & (parent == np.arange(nv)))
    number = np.full(nv, -1, np.int64)
    number[roots] = np.arange(len(roots))
    vl = np.where(used, number[parent], -1).astype(np.int32)
    pl = vl[idx[:, 0]].astype(np.int32) if len(idx) else np.empty(0, np.int32)
    return len(roots), vl, pl


def counts(nv, indices, vl, pl, C):
    """-> dict of int64 arrays (C,): vertices, primitives, edges, boundary, irregular"""
    idx = _rows(indices)
    D = idx.shape[1]
    per = lambda lab: np.bincount(lab, minlength=C).astype(np.int64)  # noqa: E731
    out = {"vertices": per(vl[vl >= 0]), "primitives": per(pl)}
    if D == 3:
        he = np.concatenate([idx[:, [0, 1]], idx[:, [1, 2]], idx[:, [2, 0]]])
        he = he[he[:, 0] != he[:, 1]]
        lo, hi = he.min(axis=1), he.max(axis=1)
        key, inv, cnt = np.unique(lo << 32 | hi, return_inverse=True, return_counts=True)
        forward = np.bincount(inv, weights=(he[:, 0] < he[:, 1]), minlength=len(key)).astype(np.int64)
        part = vl[key >> 32]
        out["edges"] = per(part)
        out["boundary"] = per(part[cnt == 1])
        out["irregular"] = per(part[(cnt > 2) | ((cnt == 2) & (forward != 1))])
    else:
        real = idx[:, 0] != idx[:, 1]
        dout = np.bincount(idx[real, 0], minlength=nv)
        din = np.bincount(idx[real, 1], minlength=nv)
        usedv = vl >= 0
        end = usedv & (din + dout == 1)
        odd = usedv & ~end & ~((din == 1) & (dout == 1))
        out["edges"] = per(pl[real])
        out["boundary"] = per(vl[end])
        out["irregular"] = per(vl[odd])
    return out


def terms(vertices, indices):
    """Per primitive, fp64 from the fp32 coordinates: (size term, enclosed term, M of the size bound, M of the enclosed
    bound).  3-D: |(b-a) x (c-a)| / 2, a . (b x c) / 6, |b-a| |c-a|, |a| |b| |c|; 2-D: |b-a|, (a_x b_y - a_y b_x) / 2,
    |b-a|, |a| |b|."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    idx = _rows(indices)
    norm = lambda x: np.sqrt((x * x).sum(axis=1))  # noqa: E731
    a, b = v[idx[:, 0]], v[idx[:, 1]]
    if idx.shape[1] == 3:
        c = v[idx[:, 2]]
        return (0.5 * norm(np.cross(b - a, c - a)), (a * np.cross(b, c)).sum(axis=1) / 6.0, norm(b - a) * norm(c - a),
                norm(a) * norm(b) * norm(c))
    return norm(b - a), 0.5 * (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), norm(b - a), norm(a) * norm(b)


def boxes(vertices, vl, C):
    """-> (lo, hi) float32 (C, ndim): the per-axis extremes of every part's vertices"""
    v = np.asarray(vertices, np.float32)
    lo = np.full((C, v.shape[1]), np.inf, np.float32)
    hi = np.full((C, v.shape[1]), -np.inf, np.float32)
    on = vl >= 0
    np.minimum.at(lo, vl[on], v[on])
    np.maximum.at(hi, vl[on], v[on])
    return lo, hi


class Parts:
    """Everything the contract says about a mesh's parts.  size / enclosed: math.fsum of the terms; size_bound /
    enclosed_bound: (P_c + 16) 2^-52 M_c, the any-order summation bound plus the terms' own roundings."""

    def __init__(self, vertices, indices):
        vertices = np.asarray(vertices, np.float32)
        nv = len(vertices)
        self.count, self.vertex_labels, self.primitive_labels = labels(nv, indices)
        C = self.count
        for k, val in counts(nv, indices, self.vertex_labels, self.primitive_labels, C).items():
            setattr(self, k, val)
        st, et, ms, me = terms(vertices, indices) if len(indices) else (np.empty(0),) * 4
        groups = [np.flatnonzero(self.primitive_labels == c) for c in range(C)]
        self.size = np.array([math.fsum(st[g]) for g in groups], np.float64)
        self.enclosed = np.array([math.fsum(et[g]) for g in groups], np.float64)
        eps = 2.0 ** -52
        self.size_bound = np.array([(len(g) + 16) * eps * math.fsum(ms[g]) for g in groups], np.float64)
        self.enclosed_bound = np.array([(len(g) + 16) * eps * math.fsum(me[g]) for g in groups], np.float64)
        self.lo, self.hi = boxes(vertices, self.vertex_labels, C) if nv else (np.empty((0, 0), np.float32),) * 2
        self.closed = (self.boundary == 0) & (self.irregular == 0)
        self.euler = self.vertices - self.edges + (self.primitives if _rows(indices).shape[1] == 3 else 0)


def select(vertices, normals, indices, keys, vl, pl, keep):
    """The sub-mesh of the parts keep marks -> (vertices, normals or None, indices, keys)"""
    keep = np.asarray(keep, bool)
    indices = _rows(indices, np.int32)
    vkeep = (vl >= 0) & keep[np.maximum(vl, 0)] if len(keep) else np.zeros(len(vl), bool)
    pkeep = keep[pl] if len(keep) else np.zeros(len(pl), bool)
    to = np.cumsum(vkeep) - 1
    idx = to[indices[pkeep]].astype(np.int32).reshape(-1, indices.shape[1])
    return (np.asarray(vertices)[vkeep], None if normals is None else np.asarray(normals)[vkeep], idx, np.asarray(keys)[vkeep])


# ---- the fields of the tests ------------------------------------------------------------------------------------------

def _grid(sizes):
    g = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sizes[::-1]], indexing="ij")
    return g[::-1]


FIXTURE_3D_SIZES = [28, 24, 20]
FIXTURE_2D_SIZES = [40, 33]
CHECKERBOARD_SIZES = [7, 8, 9]


def fixture_3d():
    """Three spheres (the last cut by the border) and a torus on [28, 24, 20]: the minimum of their distances, fp32, flat"""
    x, y, z = _grid(FIXTURE_3D_SIZES)
    sphere = lambda c, r: np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r  # noqa: E731
    torus = lambda c, R, r: np.sqrt((np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - R) ** 2 + (z - c[2]) ** 2) - r  # noqa: E731
    f = np.minimum.reduce([sphere((6.3, 6.1, 6.2), 4.1), sphere((20.2, 6.7, 13.1), 2.3), torus((15.1, 15.2, 9.3), 4.6, 1.9),
                           sphere((26.4, 20.3, 3.2), 4.1)])
    return f.astype(np.float32).reshape(-1)


def fixture_2d():
    """A disc with a hole, a small disc and a disc cut by the border on [40, 33], fp32, flat"""
    x, y = _grid(FIXTURE_2D_SIZES)
    disc = lambda c, r: np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - r  # noqa: E731
    f = np.minimum.reduce([disc((10.3, 9.2), 6.1), disc((28.7, 20.4), 3.2), disc((38.2, 5.1), 4.3)])
    f = np.maximum(f, -disc((10.3, 9.2), 2.4))
    return f.astype(np.float32).reshape(-1)


def checkerboard(sizes=None):
    """tests/test_gpu_iso.py's checkerboard: alternating signs with varying magnitudes"""
    sizes = CHECKERBOARD_SIZES if sizes is None else sizes
    g = np.indices(sizes[::-1]).sum(axis=0)
    f = np.where(g % 2 == 0, -1.0, 1.0).astype(np.float32) * (1 + 0.1 * (np.arange(g.size) % 7).reshape(g.shape))
    return f.astype(np.float32).reshape(-1)
