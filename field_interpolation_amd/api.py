"""Host-side mirror of the reference's C++ interface for the hot path, over the C ABI.

Names, argument meaning, defaults and error behaviour follow
  field_interpolation/field_interpolation.hpp:44-183 and field_interpolation/sparse_linear.hpp:8-80
so the parity tests read like calls into the reference.  Differences that the matrix-free design
forces are stated where they occur:
  * `LatticeField.eq` (the materialised triplet list, hpp:99) does not exist: rows go straight to
    the GPU, so the solver functions take the field instead of `field.eq`;
  * solvers return None where the reference returns an empty vector (sparse_linear.cpp:137-149,
    169-181, 402-405).
Buffers may be numpy arrays (host) or torch CUDA tensors (device pointers are passed through).
"""
import collections
import ctypes as C
import enum
import functools
import math

import numpy as np

from . import _capi
from ._capi import FI_DEVICE, FI_F32, FI_F64, FI_HOST, FiError, FiStats, FiWeights, check

MAX_DIM = 3  # field_interpolation.hpp:44


class ValueKernel(enum.IntEnum):      # field_interpolation.hpp:47-51
    kNearestNeighbor = 0
    kLinearInterpolation = 1


class GradientKernel(enum.IntEnum):   # field_interpolation.hpp:54-59
    kNearestNeighbor = 0
    kCellEdges = 1
    kLinearInterpolation = 2


class Weights:
    """field_interpolation.hpp:75-95, same field names and defaults."""

    def __init__(self, data_pos=1.0, data_gradient=1.0, model_0=0.0, model_1=0.0, model_2=0.5, model_3=0.0,
                 model_4=0.0, gradient_smoothness=0.0, value_kernel=ValueKernel.kLinearInterpolation,
                 gradient_kernel=GradientKernel.kCellEdges):
        self.data_pos, self.data_gradient = data_pos, data_gradient
        self.model_0, self.model_1, self.model_2 = model_0, model_1, model_2
        self.model_3, self.model_4 = model_3, model_4
        self.gradient_smoothness = gradient_smoothness
        self.value_kernel, self.gradient_kernel = value_kernel, gradient_kernel

    def _c(self):
        return FiWeights(self.data_pos, self.data_gradient, self.model_0, self.model_1, self.model_2,
                         self.model_3, self.model_4, self.gradient_smoothness, int(self.value_kernel),
                         int(self.gradient_kernel))


class SolveOptions:
    """sparse_linear.hpp:66-73."""

    def __init__(self, tile=False, tile_size=16, cg=True, max_iterations=0, error_tolerance=1e-3):
        self.tile, self.tile_size, self.cg = tile, tile_size, cg
        self.max_iterations, self.error_tolerance = max_iterations, error_tolerance


def _buf(a, dtype=np.float32):
    """(pointer, memory kind, keep-alive object) of a numpy array / torch tensor / None."""
    if a is None:
        return None, None, None
    if hasattr(a, "data_ptr"):           # torch tensor
        import torch
        want = {np.float32: torch.float32, np.float64: torch.float64, np.int32: torch.int32, np.int64: torch.int64}[dtype]
        t = a.contiguous()
        if t.dtype != want:
            t = t.to(want)
        return C.c_void_p(t.data_ptr()), (FI_DEVICE if t.is_cuda else FI_HOST), t
    arr = np.ascontiguousarray(a, dtype=dtype)
    return C.c_void_p(arr.ctypes.data), FI_HOST, arr


def _same_memory(*kinds):
    ks = {k for k in kinds if k is not None}
    if len(ks) > 1:
        raise ValueError("all buffers of one call must live in the same memory (all host or all device)")
    return ks.pop() if ks else FI_HOST


IsoMesh = collections.namedtuple("IsoMesh", ["vertices", "normals", "indices", "keys"])
IsoMesh.__doc__ = """An iso-contour (2-D: segments, indices (P, 2)) or iso-surface (3-D: triangles, indices (P, 3)) in lattice units:
vertices (V, ndim) float32, normals (V, ndim) float32 or None, indices int32, keys (V,) int64 = ndim * index(p) + axis of
the lattice edge (p, p + e_axis) each vertex lies on, ascending (include/fi_hip.h, fi_iso_extract)."""


def _take_mesh(h, ndim, normals=True):
    """IsoMesh of a device mesh handle, which is destroyed."""
    try:
        nv, np_, vpp = C.c_long(0), C.c_long(0), C.c_int(0)
        check(_capi.lib().fi_mesh_info(h, C.byref(nv), C.byref(np_), C.byref(vpp)))
        v = np.empty((nv.value, ndim), np.float32)
        n = np.empty((nv.value, ndim), np.float32) if normals else None
        i = np.empty((np_.value, vpp.value or ndim), np.int32)
        k = np.empty(nv.value, np.int64)
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
        check(_capi.lib().fi_mesh_copy(h, ptr(v), ptr(n), ptr(i), ptr(k), FI_HOST))
        return IsoMesh(v, n, i, k)
    finally:
        _capi.lib().fi_mesh_destroy(h)


MeshParts = collections.namedtuple("MeshParts", ["vertex_labels", "primitive_labels", "vertices", "primitives", "edges", "boundary",
                                                 "irregular", "size", "enclosed", "lo", "hi", "closed", "euler"])
MeshParts.__doc__ = """The connected parts of a mesh (include/fi_hip.h, fi_mesh_parts / fi_mesh_measure): vertex_labels (V,) and
primitive_labels (P,) int32, the part of every vertex (-1: used by no primitive) and primitive, parts numbered by their smallest
vertex; then one entry per part: vertices, primitives, edges, boundary, irregular (int64), size (area / length) and enclosed
(volume / area, positive for a blob of inside, negative for a cavity; meaningful for closed parts) float64, lo / hi (C, ndim)
float32 bounding boxes, closed = no boundary and nothing irregular, euler = vertices - edges + primitives (2-D, where the
segments are the edges: vertices - edges)."""


def _mesh_handle(mesh):
    """A device mesh handle (the caller destroys it) of an IsoMesh of numpy arrays or torch tensors -> (handle, ndim, memory,
    a tensor of the mesh or None)."""
    v, vmem, vkeep = _buf(mesh.vertices)
    n, nmem, _nkeep = _buf(mesh.normals)
    i, imem, ikeep = _buf(mesh.indices, np.int32)
    k, kmem, _kkeep = _buf(mesh.keys, np.int64)
    mem = _same_memory(vmem, nmem, imem, kmem)
    if len(vkeep.shape) != 2 or len(ikeep.shape) != 2 or vkeep.shape[1] != ikeep.shape[1]:
        raise ValueError("a mesh is vertices (V, ndim) and indices (P, ndim)")
    ndim = int(vkeep.shape[1])
    nv, npr = int(vkeep.shape[0]), int(ikeep.shape[0])
    for other, keep in ((n, _nkeep), (k, _kkeep)):
        if other is not None and int(keep.shape[0]) != nv:
            raise ValueError("normals and keys have one entry per vertex")
    h = C.c_void_p()
    check(_capi.lib().fi_mesh_create(C.byref(h), ndim, nv, v if nv else None, n if nv else None, k if nv else None, npr,
                                     i if npr else None, mem))
    return h, ndim, mem, (vkeep if hasattr(vkeep, "data_ptr") else None)


def _handle_parts(h, ndim, like=None):
    """MeshParts of a device mesh handle; the labels as torch tensors on like's device, else numpy."""
    L = _capi.lib()
    nv, np_, count = C.c_long(0), C.c_long(0), C.c_long(0)
    check(L.fi_mesh_info(h, C.byref(nv), C.byref(np_), None))
    if like is not None and like.is_cuda:
        import torch
        vl = torch.empty(nv.value, dtype=torch.int32, device=like.device)
        pl = torch.empty(np_.value, dtype=torch.int32, device=like.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None  # noqa: E731
        check(L.fi_mesh_parts(h, C.byref(count), ptr(vl), ptr(pl), FI_DEVICE))
    else:
        vl, pl = np.empty(nv.value, np.int32), np.empty(np_.value, np.int32)
        check(L.fi_mesh_parts(h, C.byref(count), C.c_void_p(vl.ctypes.data), C.c_void_p(pl.ctypes.data), FI_HOST))
    rows = (_capi.FiMeshPart * max(count.value, 1))()
    check(L.fi_mesh_measure(h, count.value, C.cast(rows, C.c_void_p), C.byref(count)))
    rows = rows[:count.value]
    col = lambda f, t: np.array([getattr(r, f) for r in rows], t)  # noqa: E731
    ints = {f: col(f, np.int64) for f in ("vertices", "primitives", "edges", "boundary", "irregular")}
    box = lambda f: np.array([list(getattr(r, f))[:ndim] for r in rows], np.float32).reshape(-1, ndim)  # noqa: E731
    closed = (ints["boundary"] == 0) & (ints["irregular"] == 0)
    euler = ints["vertices"] - ints["edges"] + (ints["primitives"] if ndim == 3 else 0)
    return MeshParts(vl, pl, ints["vertices"], ints["primitives"], ints["edges"], ints["boundary"], ints["irregular"],
                     col("size", np.float64), col("enclosed", np.float64), box("lo"), box("hi"), closed, euler)


def _handle_select(h, keep):
    """The sub-mesh of the parts keep marks, as a new device mesh handle."""
    keep = np.ascontiguousarray(np.asarray(keep).astype(bool), np.uint8).reshape(-1)
    out = C.c_void_p()
    check(_capi.lib().fi_mesh_select(h, len(keep), C.c_void_p(keep.ctypes.data) if len(keep) else None, C.byref(out)))
    return out


def _take_mesh_like(h, ndim, normals, like):
    """_take_mesh, or with `like` a CUDA tensor the same as torch tensors on its device."""
    if like is None or not like.is_cuda:
        return _take_mesh(h, ndim, normals)
    import torch
    try:
        nv, np_ = C.c_long(0), C.c_long(0)
        check(_capi.lib().fi_mesh_info(h, C.byref(nv), C.byref(np_), None))
        v = torch.empty((nv.value, ndim), dtype=torch.float32, device=like.device)
        n = torch.empty((nv.value, ndim), dtype=torch.float32, device=like.device) if normals else None
        i = torch.empty((np_.value, ndim), dtype=torch.int32, device=like.device)
        k = torch.empty(nv.value, dtype=torch.int64, device=like.device)
        ptr = lambda t: None if t is None or not t.numel() else C.c_void_p(t.data_ptr())  # noqa: E731
        check(_capi.lib().fi_mesh_copy(h, ptr(v), ptr(n), ptr(i), ptr(k), FI_DEVICE))
        return IsoMesh(v, n, i, k)
    finally:
        _capi.lib().fi_mesh_destroy(h)


def mesh_parts(mesh):
    """The connected parts of a mesh the caller holds (an IsoMesh of numpy arrays, or of torch CUDA tensors: then the labels
    come back as tensors on that device), labelled and measured on the device.  normals and keys may be None.  -> MeshParts"""
    h, ndim, _mem, like = _mesh_handle(mesh)
    try:
        return _handle_parts(h, ndim, like)
    finally:
        _capi.lib().fi_mesh_destroy(h)


def select_parts(mesh, keep):
    """The sub-mesh of the parts whose entry of `keep` (one boolean per part, e.g. keep_parts') is set: their vertices in the
    original order with normals and keys, their primitives in the original order with indices remapped; vertices no kept
    primitive uses are dropped.  -> IsoMesh, where `mesh` lives"""
    h, ndim, _mem, like = _mesh_handle(mesh)
    try:
        out = _handle_select(h, keep)
    finally:
        _capi.lib().fi_mesh_destroy(h)
    return _take_mesh_like(out, ndim, mesh.normals is not None, like)


def keep_parts(parts, largest=None, min_size=0.0, min_primitives=0, closed=None):
    """A boolean mask over the parts of a MeshParts: those with size >= min_size, at least min_primitives primitives and, with
    closed = True / False, those that are closed / open; with largest = k only the k of them with the largest size (ties go
    to the lower part number).  Evaluated on the host from the rows of fi_mesh_measure."""
    size = np.asarray(parts.size, np.float64)
    mask = (size >= float(min_size)) & (np.asarray(parts.primitives) >= int(min_primitives))
    if closed is not None:
        mask &= np.asarray(parts.closed) == bool(closed)
    if largest is not None:
        if int(largest) < 0:
            raise ValueError("largest must be >= 0")
        order = np.argsort(-size, kind="stable")          # descending size, ties by ascending part number
        order = order[mask[order]][:int(largest)]
        mask = np.zeros(len(size), bool)
        mask[order] = True
    return mask


FI_PLACEMENT = {"quadric": 0, "mean": 1}


def _placement(placement):
    if placement not in FI_PLACEMENT:
        raise ValueError("placement is 'quadric' or 'mean'")
    return FI_PLACEMENT[placement]


def _handle_simplify(h, ndim, cell, origin=None, placement="quadric", vertex_map=None, memory=FI_HOST):
    """The simplified mesh of a device mesh handle, as a new handle; vertex_map: a pointer to int32 per input vertex in
    `memory`, or None."""
    o = None
    if origin is not None:
        o = np.ascontiguousarray(np.asarray(origin, np.float32).reshape(-1))
        if len(o) != ndim:
            raise ValueError("origin has one entry per axis")
    out = C.c_void_p()
    check(_capi.lib().fi_mesh_simplify(h, float(cell), None if o is None else C.c_void_p(o.ctypes.data), _placement(placement),
                                       vertex_map, memory, C.byref(out)))
    return out


def _simplify_args(simplify):
    """(cell, placement) of the extractors' `simplify` keyword: a cell, or a (cell, placement) pair"""
    if isinstance(simplify, (tuple, list)):
        if len(simplify) != 2:
            raise ValueError("simplify is a cell or a (cell, placement) pair")
        return float(simplify[0]), simplify[1]
    return float(simplify), "quadric"


def simplify_mesh(mesh, cell, origin=None, placement="quadric", vertex_map=False):
    """`mesh` (an IsoMesh of numpy arrays, or of torch CUDA tensors; normals and keys may be None) made coarser on the device by
    vertex clustering: the vertices in one cube of edge `cell` (the grid starts at `origin`, default 0) become one vertex,
    placed at the minimum of the cluster's quadric error ("quadric": corners and edges survive) or at the cluster's mean
    ("mean"); primitives that collapse and repeated primitives are dropped.  With a cell below the vertex spacing this welds
    the coincident vertices of a triangle soup.  keys of the result: the clusters' cell keys, ascending (include/fi_hip.h
    fi_mesh_simplify).  -> IsoMesh where `mesh` lives; vertex_map=True: -> (IsoMesh, int32 per input vertex: its output vertex
    or -1)."""
    h, ndim, _mem, like = _mesh_handle(mesh)
    try:
        vm, vptr, mem = None, None, FI_HOST
        if vertex_map:
            nv = int(mesh.vertices.shape[0])
            if like is not None and like.is_cuda:
                import torch
                vm = torch.empty(nv, dtype=torch.int32, device=like.device)
                vptr, mem = (C.c_void_p(vm.data_ptr()) if nv else None), FI_DEVICE
            else:
                vm = np.empty(nv, np.int32)
                vptr = C.c_void_p(vm.ctypes.data) if nv else None
        out = _handle_simplify(h, ndim, cell, origin, placement, vptr, mem)
    finally:
        _capi.lib().fi_mesh_destroy(h)
    res = _take_mesh_like(out, ndim, mesh.normals is not None, like)
    return (res, vm) if vertex_map else res


FI_BOUNDARY = {"fixed": 0, "slide": 1, "free": 2}
FI_SMOOTH_NORMALS = {"recompute": 0, "keep": 1}


def _handle_smooth(h, iterations=10, lam=0.5, mu=-0.53, boundary="fixed", max_move=None, normals="recompute"):
    """The smoothed mesh of a device mesh handle, as a new handle (smooth_mesh's keywords)."""
    if boundary not in FI_BOUNDARY:
        raise ValueError("boundary is 'fixed', 'slide' or 'free'")
    if normals not in FI_SMOOTH_NORMALS:
        raise ValueError("normals is 'recompute' or 'keep'")
    opt = _capi.FiSmoothOptions(int(iterations), float(lam), float(mu), FI_BOUNDARY[boundary],
                                0.0 if max_move is None else float(max_move), FI_SMOOTH_NORMALS[normals])
    out = C.c_void_p()
    check(_capi.lib().fi_mesh_smooth(h, C.byref(opt), C.byref(out)))
    return out


def _smooth_args(smooth):
    """smooth_mesh's keywords of the extractors' `smooth` keyword: an iteration count, or a dict of them"""
    if isinstance(smooth, dict):
        return dict(smooth)
    return {"iterations": int(smooth)}


def smooth_mesh(mesh, iterations=10, lam=0.5, mu=-0.53, boundary="fixed", max_move=None, normals="recompute"):
    """`mesh` (an IsoMesh of numpy arrays, or of torch CUDA tensors; normals and keys may be None) made smoother on the device
    by Taubin's fairing with uniform weights: `iterations` times, every vertex moves towards the average of its neighbours
    by the factor lam and then by the factor mu (negative: it undoes the shrinking of the first step; mu = 0 is plain
    Laplacian smoothing).  boundary: "fixed" (the vertices of open edges stay), "slide" (they are faired along the rim) or
    "free"; max_move: no vertex ends further than this from where it started (None: no limit); normals: "recompute" (from
    the smoothed triangles, area-weighted: mesh_normals) or "keep" -- a mesh without normals stays without.  Vertex count,
    indices and keys are the input's (include/fi_hip.h fi_mesh_smooth).  -> IsoMesh where `mesh` lives"""
    h, ndim, _mem, like = _mesh_handle(mesh)
    try:
        out = _handle_smooth(h, iterations, lam, mu, boundary, max_move, normals)
    finally:
        _capi.lib().fi_mesh_destroy(h)
    return _take_mesh_like(out, ndim, mesh.normals is not None, like)


def mesh_normals(mesh):
    """`mesh` with vertex normals computed on the device from its primitives: the area- (2-D: length-) weighted sum of the
    normals of the primitives around each vertex, normalised, pointing from the extractors' inside to their outside; zeros
    for a vertex no primitive uses (include/fi_hip.h fi_mesh_normals).  Works on a mesh that has no normals.  -> IsoMesh
    where `mesh` lives"""
    h, ndim, _mem, like = _mesh_handle(mesh)
    try:
        out = C.c_void_p()
        check(_capi.lib().fi_mesh_normals(h, C.byref(out)))
    finally:
        _capi.lib().fi_mesh_destroy(h)
    return _take_mesh_like(out, ndim, True, like)


def _finish_mesh(h, ndim, normals, largest, min_size, parts, simplify=None, smooth=None):
    """What the extractors return for a device mesh handle: the mesh, filtered on the device if largest / min_size ask for
    it (label -> measure -> select), then smoothed on the device if `smooth` asks for it (an iteration count, or a dict of
    smooth_mesh's keywords), then simplified on the device if `simplify` asks for it (a cell, or a (cell, placement) pair),
    with one copy at the end, and with parts=True the MeshParts of the mesh returned."""
    if largest is None and min_size is None and not parts and simplify is None and smooth is None:
        return _take_mesh(h, ndim, normals)
    try:
        if largest is not None or min_size is not None:
            keep = keep_parts(_handle_parts(h, ndim), largest=largest, min_size=0.0 if min_size is None else min_size)
            kept = _handle_select(h, keep)
            _capi.lib().fi_mesh_destroy(h)
            h = kept
        if smooth is not None:
            faired = _handle_smooth(h, **_smooth_args(smooth))
            _capi.lib().fi_mesh_destroy(h)
            h = faired
        if simplify is not None:
            cell, placement = _simplify_args(simplify)
            coarse = _handle_simplify(h, ndim, cell, None, placement)
            _capi.lib().fi_mesh_destroy(h)
            h = coarse
        described = _handle_parts(h, ndim) if parts else None
    except BaseException:
        _capi.lib().fi_mesh_destroy(h)
        raise
    mesh = _take_mesh(h, ndim, normals)
    return (mesh, described) if parts else mesh


def merge_meshes(pieces):
    """The pieces of a slab decomposition (rank order) as one mesh: vertices de-duplicated by key, indices remapped."""
    pieces = list(pieces)
    keys = np.concatenate([p.keys for p in pieces])
    uniq, first = np.unique(keys, return_index=True)
    verts = np.concatenate([p.vertices for p in pieces])[first]
    normals = None
    if all(p.normals is not None for p in pieces):
        normals = np.concatenate([p.normals for p in pieces])[first]
    idx = [np.searchsorted(uniq, p.keys)[p.indices].astype(np.int32) for p in pieces]
    vpp = pieces[0].indices.shape[1] if pieces else 3
    idx = np.concatenate(idx) if idx else np.empty((0, vpp), np.int32)
    return IsoMesh(verts, normals, idx.reshape(-1, vpp), uniq.astype(np.int64))


def _sample(call, ndim, positions, other_memory, gradients, cubic, fill):
    """Shared body of the point queries: call(n, positions, mode, fill, values, gradients, memory) is the C entry point.
    Outputs live where `positions` lives: numpy in, numpy out; a torch tensor in, torch tensors out on its device."""
    p, pmem, pkeep = _buf(positions)
    count = pkeep.numel() if hasattr(pkeep, "numel") else pkeep.size
    if count % ndim:
        raise ValueError("positions: %d values, not a multiple of ndim = %d (x fastest)" % (count, ndim))
    n = count // ndim
    mem = _same_memory(pmem, *other_memory)
    if hasattr(pkeep, "data_ptr"):
        import torch
        vals = torch.empty(n, dtype=torch.float32, device=pkeep.device)
        grads = torch.empty((n, ndim), dtype=torch.float32, device=pkeep.device) if gradients else None
        if n == 0:      # (an empty tensor has no storage to point at)
            return (vals, grads) if gradients else vals
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    else:
        vals = np.empty(n, np.float32)
        grads = np.empty((n, ndim), np.float32) if gradients else None
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    check(call(n, p, 1 if cubic else 0, float(fill), ptr(vals), ptr(grads), mem))
    return (vals, grads) if gradients else vals


def _nearest(call, ndim, queries, max_distance, indices):
    """Shared body of the nearest-point queries: call(n, queries, max_distance, distances, indices, memory) is the C entry
    point.  Outputs live where `queries` lives: numpy in, numpy out; a torch tensor in, torch tensors out on its device."""
    q, qmem, qkeep = _buf(queries)
    count = qkeep.numel() if hasattr(qkeep, "numel") else qkeep.size
    if count % ndim:
        raise ValueError("queries: %d values, not a multiple of ndim = %d (x fastest)" % (count, ndim))
    n = count // ndim
    if hasattr(qkeep, "data_ptr"):
        import torch
        dist = torch.empty(n, dtype=torch.float32, device=qkeep.device)
        idx = torch.empty(n, dtype=torch.int64, device=qkeep.device) if indices else None
        if n == 0:      # (an empty tensor has no storage to point at)
            return (dist, idx) if indices else dist
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    else:
        dist = np.empty(n, np.float32)
        idx = np.empty(n, np.int64) if indices else None
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    check(call(n, q, float(max_distance), ptr(dist), ptr(idx), qmem))
    return (dist, idx) if indices else dist


def _knn(call, ndim, queries, k, max_distance, indices):
    """Shared body of the k-nearest-point queries: call(n, queries, k, max_distance, distances, indices, memory) is the C
    entry point.  Outputs (n, k) live where `queries` lives, as in _nearest."""
    q, qmem, qkeep = _buf(queries)
    count = qkeep.numel() if hasattr(qkeep, "numel") else qkeep.size
    if count % ndim:
        raise ValueError("queries: %d values, not a multiple of ndim = %d (x fastest)" % (count, ndim))
    n, k = count // ndim, int(k)
    if not 1 <= k <= 32:
        raise ValueError("k must be 1..32 (got %d)" % k)
    if hasattr(qkeep, "data_ptr"):
        import torch
        dist = torch.empty((n, k), dtype=torch.float32, device=qkeep.device)
        idx = torch.empty((n, k), dtype=torch.int64, device=qkeep.device) if indices else None
        if n == 0:      # (an empty tensor has no storage to point at)
            return (dist, idx) if indices else dist
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    else:
        dist = np.empty((n, k), np.float32)
        idx = np.empty((n, k), np.int64) if indices else None
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    check(call(n, q, k, float(max_distance), ptr(dist), ptr(idx), qmem))
    return (dist, idx) if indices else dist


def _cloud_out(device, shape, dtype):
    """an uninitialised output of `shape`: a torch tensor on `device` (a torch device or its name), or with None a numpy array
    -> (array, pointer or None for an empty one)"""
    if device is not None:
        import torch
        t = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=device)
        return t, (C.c_void_p(t.data_ptr()) if t.numel() else None)
    a = np.empty(shape, dtype)
    return a, (C.c_void_p(a.ctypes.data) if a.size else None)


def _as_mask(keep):
    """the uint8 flags of a C call as booleans"""
    return keep.bool() if hasattr(keep, "data_ptr") else keep.view(np.bool_)


def _radius_count(call, ndim, queries, radius, limit):
    """Shared body of the radius counts: call(n, queries, radius, limit, counts, memory) is the C entry point.  The counts
    live where `queries` lives."""
    q, qmem, qkeep = _buf(queries)
    count = qkeep.numel() if hasattr(qkeep, "numel") else qkeep.size
    if count % ndim:
        raise ValueError("queries: %d values, not a multiple of ndim = %d (x fastest)" % (count, ndim))
    n = count // ndim
    counts, p = _cloud_out(qkeep.device if qmem == FI_DEVICE else None, (n,), np.int32)
    if n:
        check(call(n, q, float(radius), int(limit), p, qmem))
    return counts


def _check_k(k):
    if not 1 <= int(k) <= 32:
        raise ValueError("k must be 1..32 (got %d)" % k)
    return int(k)


def _neighbour_distances(call, n, k, max_distance, device):
    """Shared body: call(k, max_distance, mean, kth, counts, memory) is the C entry point -> (mean, kth, counts)"""
    k = _check_k(k)
    dev = "cuda" if device else None
    mean, pm = _cloud_out(dev, (n,), np.float32)
    kth, pk = _cloud_out(dev, (n,), np.float32)
    counts, pc = _cloud_out(dev, (n,), np.int32)
    if n:
        check(call(k, float(max_distance), pm, pk, pc, FI_DEVICE if device else FI_HOST))
    return mean, kth, counts


def _statistical_outliers(call, n, k, std_ratio, max_distance, device):
    """Shared body: call(k, max_distance, std_ratio, keep, stats, memory) is the C entry point -> (keep, stats dict)"""
    k = _check_k(k)
    keep, pk = _cloud_out("cuda" if device else None, (n,), np.uint8)
    s = _capi.FiOutlierStats()
    check(call(k, float(max_distance), float(std_ratio), pk, C.byref(s), FI_DEVICE if device else FI_HOST))
    return _as_mask(keep), {"counted": int(s.counted), "kept": int(s.kept), "mean": float(s.mean), "stddev": float(s.stddev),
                            "threshold": float(s.threshold)}


def _radius_outliers(call, n, radius, min_neighbours, device):
    """Shared body: call(radius, min_neighbours, keep, num_kept, memory) is the C entry point -> (keep, how many are kept)"""
    keep, pk = _cloud_out("cuda" if device else None, (n,), np.uint8)
    kept = C.c_long(0)
    check(call(float(radius), int(min_neighbours), pk, C.byref(kept), FI_DEVICE if device else FI_HOST))
    return _as_mask(keep), int(kept.value)


def _cluster(call, n, eps, min_points, core, stats, device):
    """Shared body: call(eps, min_points, labels, core, stats, memory) is the C entry point -> labels, or a tuple of labels
    and what was asked for (core mask, stats dict)"""
    dev = "cuda" if device else None
    labels, pl = _cloud_out(dev, (n,), np.int32)
    flags, pc = _cloud_out(dev, (n,), np.uint8) if core else (None, None)
    s = _capi.FiClusterStats()
    check(call(float(eps), int(min_points), pl, pc, C.byref(s), FI_DEVICE if device else FI_HOST))
    out = (labels,)
    if core:
        out += (_as_mask(flags),)
    if stats:
        out += ({"clusters": int(s.clusters), "core": int(s.core), "border": int(s.border), "noise": int(s.noise),
                 "non_finite": int(s.non_finite)},)
    return out if len(out) > 1 else labels


def _estimate_normals(call, ndim, n, k, max_distance, viewpoints, directions, variation, device):
    """Shared body of the normal estimation: call(k, max_distance, orient, guides, num_guides, normals, variation, memory)
    is the C entry point.  Outputs are numpy arrays, or torch tensors on the GPU when the guides are device tensors or with
    device=True."""
    if viewpoints is not None and directions is not None:
        raise ValueError("viewpoints or directions, not both")
    guides = viewpoints if viewpoints is not None else directions
    orient = 0 if guides is None else (1 if viewpoints is not None else 2)
    g, gmem, gkeep = _buf(guides)
    ng = 0
    if guides is not None:
        count = gkeep.numel() if hasattr(gkeep, "numel") else gkeep.size
        if count % ndim:
            raise ValueError("guides: %d values, not a multiple of ndim = %d (x fastest)" % (count, ndim))
        ng = count // ndim
    on_device = device or gmem == FI_DEVICE
    if on_device:
        import torch
        if guides is not None and gmem != FI_DEVICE:
            gkeep = torch.as_tensor(gkeep).to("cuda")
            g = C.c_void_p(gkeep.data_ptr())
        dev = gkeep.device if guides is not None else "cuda"
        nrm = torch.empty((n, ndim), dtype=torch.float32, device=dev)
        var = torch.empty(n, dtype=torch.float32, device=dev) if variation else None
        ptr = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())  # noqa: E731
    else:
        nrm = np.empty((n, ndim), np.float32)
        var = np.empty(n, np.float32) if variation else None
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    if n > 0 or not on_device:
        check(call(int(k), float(max_distance), orient, g, ng, ptr(nrm), ptr(var), FI_DEVICE if on_device else FI_HOST))
    return (nrm, var) if variation else nrm


def _orient_normals(call, ndim, n, normals, k, max_distance, viewpoints, directions, components, device):
    """Shared body of the normal orientation: call(k, max_distance, anchor, guides, num_guides, normals, components, memory)
    is the C entry point.  Works on a copy of `normals`: a numpy array, or a torch tensor on the GPU when the normals or the
    guides are device tensors or with device=True."""
    if viewpoints is not None and directions is not None:
        raise ValueError("viewpoints or directions, not both")
    guides = viewpoints if viewpoints is not None else directions
    anchor = 0 if guides is None else (1 if viewpoints is not None else 2)
    g, gmem, gkeep = _buf(guides)
    ng = 0
    if guides is not None:
        count = gkeep.numel() if hasattr(gkeep, "numel") else gkeep.size
        if count % ndim:
            raise ValueError("guides: %d values, not a multiple of ndim = %d (x fastest)" % (count, ndim))
        ng = count // ndim
    _, nmem, nkeep = _buf(normals)
    count = nkeep.numel() if hasattr(nkeep, "numel") else nkeep.size
    if count != n * ndim:
        raise ValueError("normals: %d values for %d points of %d dimensions" % (count, n, ndim))
    on_device = device or gmem == FI_DEVICE or nmem == FI_DEVICE
    if on_device:
        import torch
        if guides is not None and gmem != FI_DEVICE:
            gkeep = torch.as_tensor(gkeep).to("cuda")
            g = C.c_void_p(gkeep.data_ptr())
        nrm = nkeep.clone() if nmem == FI_DEVICE else torch.as_tensor(nkeep).to(gkeep.device if guides is not None else "cuda")
        nrm = nrm.reshape(n, ndim)
        comp = torch.empty(n, dtype=torch.int64, device=nrm.device) if components else None
        ptr = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())  # noqa: E731
    else:
        nrm = np.array(nkeep, np.float32).reshape(n, ndim)
        comp = np.empty(n, np.int64) if components else None
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    if n > 0 or not on_device:
        check(call(int(k), float(max_distance), anchor, g, ng, ptr(nrm), ptr(comp), FI_DEVICE if on_device else FI_HOST))
    return (nrm, comp) if components else nrm


def _propagated(index, call, ndim, n, k, max_distance, viewpoints, directions, variation, device):
    """estimate_normals(propagate=True) of a PointIndex or a LatticeField: the canonical normals, then their orientation,
    the guides as votes"""
    if viewpoints is not None and directions is not None:
        raise ValueError("viewpoints or directions, not both")
    on_device = device or any(hasattr(g, "is_cuda") and g.is_cuda for g in (viewpoints, directions))
    res = _estimate_normals(call, ndim, n, k, max_distance, None, None, variation, on_device)
    nrm, var = res if variation else (res, None)
    nrm = index.orient_normals(nrm, k=k, max_distance=max_distance, viewpoints=viewpoints, directions=directions,
                               device=on_device)
    return (nrm, var) if variation else nrm


_MLS_DOC = """(positions (n, ndim), normals (n, ndim)) float32 -- with curvature=True also the curvature (n,) float32, with
        order=True also the order (n,) uint8, in that order -- of %s, each projected onto the surface fitted to its k nearest
        points of the set within `radius` (moving least squares, weights (1 - d^2 / radius^2)^3): degree=1 a plane, degree=2 a
        quadric over the plane's frame, in fp64 on the device.  The normal is the fitted surface's at the projected point, with
        the sign that makes its largest component positive -- or, with normals= (n, ndim) given, the sign that agrees with
        them, which is how normals oriented by orient_normals come back oriented; the curvature is the mean curvature (2-D:
        the curve's) in 1 / length, positive where the surface bends towards the normal.  order says what was fitted: 2 the
        quadric, 1 the plane (asked for, or because the neighbours do not determine a quadric), 0 nothing -- fewer than ndim
        neighbours with a positive weight, or a non-finite point: such a point stays where it is with a zero normal and a NaN
        curvature.  max_move limits how far a point may go.  The plane shrinks curved surfaces; the quadric does not, but it
        needs neighbours: with k = 16 on a noisy surface it amplifies the noise, so keep k = 32 for degree 2, and a radius
        that holds that many.  1 <= k <= 32.  The set itself is not changed: to go on with the smoothed cloud build a new
        PointIndex from the positions.  numpy arrays, or torch tensors on the GPU %s (include/fi_hip.h
        fi_mls_project)."""


def _mls_project(call, ndim, n_own, queries, k, radius, degree, max_move, normals, curvature, order, device):
    """Shared body of the moving-least-squares projection: call(n, queries, k, radius, degree, max_move, guides, positions,
    normals, curvature, order, memory) is the C entry point; queries None: the set's own n_own points."""
    k = _check_k(k)
    if degree not in (1, 2):
        raise ValueError("degree must be 1 or 2 (got %r)" % (degree,))
    q, qmem, qkeep = _buf(queries)
    if queries is None:
        n = n_own
    else:
        count = qkeep.numel() if hasattr(qkeep, "numel") else qkeep.size
        if count % ndim:
            raise ValueError("queries: %d values, not a multiple of ndim = %d (x fastest)" % (count, ndim))
        n = count // ndim
    g, gmem, gkeep = _buf(normals)
    if normals is not None:
        count = gkeep.numel() if hasattr(gkeep, "numel") else gkeep.size
        if count != n * ndim:
            raise ValueError("normals: %d values for %d points of %d dimensions" % (count, n, ndim))
    on_device = bool(device) or qmem == FI_DEVICE or gmem == FI_DEVICE
    dev = None
    if on_device:
        import torch
        dev = qkeep.device if qmem == FI_DEVICE else (gkeep.device if gmem == FI_DEVICE else "cuda")
        if queries is not None and qmem != FI_DEVICE:
            qkeep = torch.as_tensor(qkeep).to(dev)
            q = C.c_void_p(qkeep.data_ptr())
        if normals is not None and gmem != FI_DEVICE:
            gkeep = torch.as_tensor(gkeep).to(dev)
            g = C.c_void_p(gkeep.data_ptr())
    pos, pp = _cloud_out(dev, (n, ndim), np.float32)
    nrm, pn = _cloud_out(dev, (n, ndim), np.float32)
    cur, pc = _cloud_out(dev, (n,), np.float32) if curvature else (None, None)
    odr, po = _cloud_out(dev, (n,), np.uint8) if order else (None, None)
    if n:
        check(call(n, q, k, float(radius), int(degree), float(max_move), g, pp, pn, pc, po, FI_DEVICE if on_device else FI_HOST))
    return (pos, nrm) + tuple(a for a in (cur, odr) if a is not None)


def _distance_field(call, total, indices, device):
    """Shared body of the distance fields: call(distances, indices, memory); numpy arrays of `total` values (x fastest), or
    torch tensors on the current GPU with device=True."""
    if device:
        import torch
        dist = torch.empty(total, dtype=torch.float32, device="cuda")
        idx = torch.empty(total, dtype=torch.int64, device="cuda") if indices else None
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        mem = FI_DEVICE
    else:
        dist = np.empty(total, np.float32)
        idx = np.empty(total, np.int64) if indices else None
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
        mem = FI_HOST
    check(call(ptr(dist), ptr(idx), mem))
    return (dist, idx) if indices else dist


class _PointQueries:
    """The operations on a point set, once for the two classes that have one.  "The set" is, on a PointIndex, its own rows;
    on a LatticeField, the data points of the context: every add_points batch in the order they were added, the border
    prior's rows left out.  num_points below is their number (PointIndex.num_points, LatticeField.point_count()), and a
    point's index is its place in that order.  A context's search structure is built at the first call that needs it and
    kept until the next add_points / clear_points; slab contexts refuse (a rank sees only its own points).

    A class supplies _point_op(op) -- the C function fi_<op> or fi_points_<op> bound to its handle -- _point_ndim() and
    _point_count()."""

    def nearest(self, queries, max_distance=math.inf, indices=False):
        """Distances (n,) float32 -- and with indices=True also the indices (n,) int64 -- of the nearest point of the set to
        each of `queries` (n x ndim): +inf / -1 beyond max_distance or with no finite point, NaN / -1 for a non-finite query
        (include/fi_hip.h fi_nearest)."""
        return _nearest(self._point_op("nearest"), self._point_ndim(), queries, max_distance, indices)

    def knn(self, queries, k, max_distance=math.inf, indices=True):
        """Distances (n, k) float32 and, with indices=True, indices (n, k) int64 of the k nearest points of the set to each
        of `queries` (n x ndim), nearest first, equal distances by ascending index; 1 <= k <= 32.  Entries that do not exist
        (fewer than k finite points, beyond max_distance) are +inf / -1 at the end; a non-finite query gets NaN / -1.  A
        point of the set finds itself (include/fi_hip.h fi_knn)."""
        return _knn(self._point_op("knn"), self._point_ndim(), queries, k, max_distance, indices)

    def estimate_normals(self, k=16, max_distance=math.inf, viewpoints=None, directions=None, variation=False, device=False,
                         propagate=False):
        """Normals (num_points, ndim) float32 of the set's points, each fitted to its k nearest points (itself included)
        within max_distance by a local PCA in fp64 on the device; with variation=True also the surface variation
        lambda_min / sum(lambda) (num_points,).  viewpoints: one sensor position (ndim,) or one per point -- normals look
        at it (outward: the sign sdf_from_points wants); directions: rough normals, one per point, to agree with; neither:
        each normal's largest component is positive, which is NOT a consistent orientation.  Points that are non-finite or
        have fewer than ndim neighbours get a zero normal and a NaN variation (include/fi_hip.h fi_estimate_normals).
        propagate=True: the canonical normals, then orient_normals(k, max_distance) over them -- a consistent orientation
        without guides; viewpoints / directions then only vote for each component's sign."""
        args = (self._point_op("estimate_normals"), self._point_ndim(), self._point_count(), k, max_distance, viewpoints, directions,
                variation, device)
        return _propagated(self, *args) if propagate else _estimate_normals(*args)

    def orient_normals(self, normals, k=16, max_distance=math.inf, viewpoints=None, directions=None, components=False,
                       device=False):
        """`normals` (num_points, ndim) with one consistent sign per connected component of the set's k-nearest-neighbour
        graph: signs spread along the minimum spanning forest that prefers parallel normal lines (Hoppe et al.), found on
        the device; with components=True also each point's component (its smallest point index; -1 for a point that is
        non-finite or has a zero or non-finite normal, which stays as it is).  Without guides a component's highest point
        on the last axis looks up that axis; viewpoints / directions (as for estimate_normals) vote per component instead,
        so one sensor position serves a whole closed object (include/fi_hip.h fi_orient_normals)."""
        return _orient_normals(self._point_op("orient_normals"), self._point_ndim(), self._point_count(), normals, k, max_distance,
                               viewpoints, directions, components, device)

    def radius_count(self, queries, radius, limit=2 ** 31 - 1):
        """How many finite points of the set lie within `radius` of each of `queries` (n x ndim), a point exactly on the
        radius included: (n,) int32 where `queries` lives, -1 for a non-finite query.  The search of a query stops at `limit`
        points and reports `limit`: pass the number you need to know about (include/fi_hip.h fi_radius_count)."""
        return _radius_count(self._point_op("radius_count"), self._point_ndim(), queries, radius, limit)

    def neighbour_distances(self, k=8, max_distance=math.inf, device=False):
        """(mean, kth, counts), each (num_points,): the mean distance of every point of the set to its k nearest OTHER points
        within max_distance (the point itself is left out by its index; a duplicate of it is a neighbour at distance 0), the
        distance to the last of them, and how many they are.  No neighbour: +inf, +inf, 0; a non-finite point: NaN, NaN, 0.
        1 <= k <= 32.  This is also the density weight: mean ** ndim or kth ** ndim is what a caller passes on as
        `point_weights` so that an over-sampled patch does not outweigh the rest of the fit.  numpy arrays, or torch tensors
        on the GPU with device=True (include/fi_hip.h fi_neighbour_distances)."""
        return _neighbour_distances(self._point_op("neighbour_distances"), self._point_count(), k, max_distance, device)

    def smooth(self, k=32, radius=None, degree=2, max_move=math.inf, normals=None, curvature=False, order=False, device=False):
        if radius is None:
            raise ValueError("smooth needs a radius")
        return _mls_project(self._point_op("mls_project"), self._point_ndim(), self._point_count(), None, k, radius, degree, max_move,
                            normals, curvature, order, device)
    smooth.__doc__ = _MLS_DOC % ("the set's points (num_points of them, a point being its own neighbour)",
                                 "when `normals` is a device tensor or with device=True")

    def project(self, queries, k=32, radius=None, degree=2, max_move=math.inf, normals=None, curvature=False, order=False,
                device=False):
        if radius is None:
            raise ValueError("project needs a radius")
        return _mls_project(self._point_op("mls_project"), self._point_ndim(), self._point_count(), queries, k, radius, degree,
                            max_move, normals, curvature, order, device)
    project.__doc__ = _MLS_DOC % ("`queries` (n x ndim: any points -- a grid to resample a scan on, or more points than it has)",
                                  "when `queries` or `normals` is a device tensor or with device=True")

    def statistical_outliers(self, k=8, std_ratio=2.0, max_distance=math.inf, device=False):
        """The statistical outlier rule of PCL and Open3D: a point is kept when its mean distance to its k nearest other
        points (neighbour_distances) is at most mean + std_ratio * standard deviation of that figure over the cloud, the two
        summed in a fixed order.  -> (keep (num_points,) bool, stats: counted, kept, mean, stddev, threshold); points that are
        non-finite or have no neighbour within max_distance are neither counted nor kept (include/fi_hip.h
        fi_outliers_statistical)."""
        return _statistical_outliers(self._point_op("outliers_statistical"), self._point_count(), k, std_ratio, max_distance, device)

    def radius_outliers(self, radius, min_neighbours=2, device=False):
        """-> (keep (num_points,) bool, how many are kept): a point is kept when it is finite and at least min_neighbours
        other finite points lie within `radius` of it (include/fi_hip.h fi_outliers_radius)."""
        return _radius_outliers(self._point_op("outliers_radius"), self._point_count(), radius, min_neighbours, device)

    def cluster(self, eps, min_points=1, core=False, stats=False, device=False):
        """Labels (num_points,) int32 of the clusters of the set's points (include/fi_hip.h fi_cluster): a point
        is CORE when at least min_points points of the set, itself included, lie within eps of it (a point exactly at eps
        counts); core points within eps of each other share a cluster, and clusters are numbered by their lowest core point; a
        point that is not core takes the cluster of its nearest core point within eps (ties: the lower index), and -1 (noise)
        without one; a non-finite point gets -1.  min_points = 1: plain Euclidean clustering, every finite point in a cluster.
        core=True adds the core mask (bool), stats=True a dict: clusters, core, border, noise, non_finite.  numpy arrays, or
        torch tensors on the GPU with device=True.  An eps that spans the cloud makes every point visit every other: slow."""
        return _cluster(self._point_op("cluster"), self._point_count(), eps, min_points, core, stats, device)


class PointIndex(_PointQueries):
    """Exact nearest points of a point set of its own, searched on the device (include/fi_hip.h fi_points_create; the
    contract is fi_nearest's).  positions: (n, ndim) -- or (n,) in 1-D -- numpy array or torch tensor, x fastest; a point's
    index is its row."""

    def __init__(self, positions, ndim=None):
        p, mem, keep = _buf(positions)
        shape = tuple(keep.shape)
        self.ndim = int(ndim) if ndim is not None else (shape[-1] if len(shape) == 2 else 1)
        count = keep.numel() if hasattr(keep, "numel") else keep.size
        if count % self.ndim:
            raise ValueError("positions: %d values, not a multiple of ndim = %d (x fastest)" % (count, self.ndim))
        self.num_points = count // self.ndim
        self._h = C.c_void_p()
        check(_capi.lib().fi_points_create(C.byref(self._h), self.ndim, self.num_points, p if count else None, mem))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _capi._LIB is not None:
            _capi._LIB.fi_points_destroy(h)
        self._h = None

    def _point_op(self, op):
        return functools.partial(getattr(_capi.lib(), "fi_points_" + op), self._h)

    def _point_ndim(self):
        return self.ndim

    def _point_count(self):
        return self.num_points

    def describe(self, normals, k=32, max_distance=math.inf, device=False):
        """(features (num_points, 33) float32, valid (num_points,) bool): what every point's neighbourhood looks like as a
        fast point feature histogram (Rusu) over its k nearest points within max_distance and the normals (num_points, 3)
        -- three blocks of 11 bins that each sum to 100 and do not change when the cloud is turned or shifted, which is what
        match_features compares.  A point that is non-finite, has a zero or non-finite normal or no usable neighbour gets
        zeros and valid = False.  3-D sets only; 1 <= k <= 32.  numpy arrays, or torch tensors on the GPU when `normals` is a
        device tensor or with device=True (include/fi_hip.h fi_points_describe)."""
        k = _check_k(k)
        n = self.num_points
        nrm, nmem, nkeep = _buf(normals)
        count = nkeep.numel() if hasattr(nkeep, "numel") else nkeep.size
        if count != n * 3:
            raise ValueError("normals: %d values for %d points of 3 dimensions" % (count, n))
        on_device = bool(device) or nmem == FI_DEVICE
        if on_device and nmem != FI_DEVICE:
            import torch
            nkeep = torch.as_tensor(nkeep).to("cuda")
            nrm = C.c_void_p(nkeep.data_ptr())
        dev = (nkeep.device if on_device else None)
        feat, pf = _cloud_out(dev, (n, 33), np.float32)
        valid, pv = _cloud_out(dev, (n,), np.uint8)
        if n:
            check(_capi.lib().fi_points_describe(self._h, nrm, k, float(max_distance), pf, pv, FI_DEVICE if on_device else FI_HOST))
        return feat, _as_mask(valid)

    def distance_field(self, sizes, max_distance=math.inf, indices=False, device=False):
        """PointIndex.nearest of every point of a lattice of `sizes` (x fastest), flat."""
        if len(sizes) != self.ndim:
            raise ValueError("sizes: %d extents for a %d-D point set" % (len(sizes), self.ndim))
        sz = (C.c_int * len(sizes))(*[int(s) for s in sizes])

        def call(d, i, mem):
            return _capi.lib().fi_points_distance_field(self._h, sz, float(max_distance), d, i, mem)
        return _distance_field(call, int(np.prod(sizes)), indices, device)


_SURFACE_METHODS = {"iso": 0, "dual": 1}     # FI_SURFACE_ISO, FI_SURFACE_DUAL


def _surface_method(method):
    if method not in _SURFACE_METHODS:
        raise ValueError("method must be 'iso' (fi_iso_extract's mesh) or 'dual' (fi_dual_contour's), not %r" % (method,))
    return _SURFACE_METHODS[method]


def _redistance(call, total, primitives, device, ndim):
    """Shared body of the redistancing calls: call(out, primitives, mesh handle pointer, memory).  -> distances, or with
    primitives=True (distances, primitive indices, the IsoMesh they index)"""
    if not primitives:
        return _distance_field(lambda d, i, mem: call(d, None, None, mem), total, False, device)
    h = C.c_void_p()
    try:
        d, i = _distance_field(lambda d, i, mem: call(d, i, C.byref(h), mem), total, True, device)
    except BaseException:
        if h:
            _capi.lib().fi_mesh_destroy(h)
        raise
    return d, i, _take_mesh(h, ndim)


class SurfaceIndex:
    """Exact distances to a mesh of its own, searched on the device (include/fi_hip.h fi_surface_create): 2-D segments or 3-D
    triangles.  vertices: (V, ndim) float32 in lattice units, indices: (P, ndim) int32 -- numpy arrays or torch tensors in
    the same memory; a primitive's index is its row."""

    def __init__(self, vertices, indices):
        v, vmem, vkeep = _buf(vertices)
        i, imem, ikeep = _buf(indices, np.int32)
        mem = _same_memory(vmem, imem)
        vshape, ishape = tuple(vkeep.shape), tuple(ikeep.shape)
        self.ndim = int(ishape[-1]) if len(ishape) == 2 else int(vshape[-1])
        vcount = vkeep.numel() if hasattr(vkeep, "numel") else vkeep.size
        icount = ikeep.numel() if hasattr(ikeep, "numel") else ikeep.size
        if vcount % self.ndim or icount % self.ndim:
            raise ValueError("vertices / indices: %d / %d values, not multiples of ndim = %d" % (vcount, icount, self.ndim))
        self.num_vertices, self.num_primitives = vcount // self.ndim, icount // self.ndim
        self._h = C.c_void_p()
        check(_capi.lib().fi_surface_create(C.byref(self._h), self.ndim, self.num_vertices, v if vcount else None,
                                            self.num_primitives, i if icount else None, mem))

    @classmethod
    def from_mesh(cls, mesh):
        """The surface of an IsoMesh (LatticeField.iso_surface / dual_contour, iso_surface, dual_contour)"""
        return cls(mesh.vertices, mesh.indices)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _capi._LIB is not None:
            _capi._LIB.fi_surface_destroy(h)
        self._h = None

    def distance(self, queries, max_distance=math.inf, primitives=False, closest=False):
        """Distances (n,) float32 from each of `queries` (n x ndim) to the surface; with primitives=True also the nearest
        primitive (n,) int64, with closest=True also the closest point (n, ndim) float32 -- a tuple in that order.  Beyond
        max_distance or with no usable primitive: +inf, -1, NaN; a non-finite query: NaN, -1, NaN.  Outputs live where
        `queries` lives (include/fi_hip.h fi_surface_distance)."""
        q, qmem, qkeep = _buf(queries)
        count = qkeep.numel() if hasattr(qkeep, "numel") else qkeep.size
        if count % self.ndim:
            raise ValueError("queries: %d values, not a multiple of ndim = %d (x fastest)" % (count, self.ndim))
        n = count // self.ndim
        if hasattr(qkeep, "data_ptr"):
            import torch
            dist = torch.empty(n, dtype=torch.float32, device=qkeep.device)
            idx = torch.empty(n, dtype=torch.int64, device=qkeep.device) if primitives else None
            cl = torch.empty((n, self.ndim), dtype=torch.float32, device=qkeep.device) if closest else None
            ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        else:
            dist = np.empty(n, np.float32)
            idx = np.empty(n, np.int64) if primitives else None
            cl = np.empty((n, self.ndim), np.float32) if closest else None
            ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
        if n:   # (an empty tensor has no storage to point at)
            check(_capi.lib().fi_surface_distance(self._h, n, q, float(max_distance), ptr(dist), ptr(idx), ptr(cl), qmem))
        out = tuple(a for a in (dist, idx, cl) if a is not None)
        return out if len(out) > 1 else dist

    def distance_field(self, sizes, max_distance=math.inf, primitives=False, device=False):
        """SurfaceIndex.distance of every point of a lattice of `sizes` (x fastest), flat, unsigned: numpy arrays, or torch
        tensors with device=True."""
        if len(sizes) != self.ndim:
            raise ValueError("sizes: %d extents for a %d-D surface" % (len(sizes), self.ndim))
        sz = (C.c_int * len(sizes))(*[int(s) for s in sizes])

        def call(d, i, mem):
            return _capi.lib().fi_surface_distance_field(self._h, sz, float(max_distance), d, i, mem)
        return _distance_field(call, int(np.prod(sizes)), primitives, device)

    # ---- rays (include/fi_hip.h fi_surface_raycast) ----
    def _rows(self, what, a):
        """(pointer, memory, keep-alive, rows) of an (n, ndim) float32 input"""
        p, mem, keep = _buf(a)
        count = keep.numel() if hasattr(keep, "numel") else keep.size
        if count % self.ndim:
            raise ValueError("%s: %d values, not a multiple of ndim = %d (x fastest)" % (what, count, self.ndim))
        return p, mem, keep, count // self.ndim

    def _rays(self, origins, directions):
        o, omem, okeep, n = self._rows("origins", origins)
        d, dmem, dkeep, nd = self._rows("directions", directions)
        if nd != n:
            raise ValueError("%d origins, %d directions" % (n, nd))
        return o, d, _same_memory(omem, dmem), (okeep, dkeep), n

    @staticmethod
    def _like(keep, shape, dtype):
        """an output of `shape` where the input `keep` lives, and its pointer"""
        if hasattr(keep, "data_ptr"):
            import torch
            out = torch.empty(shape, dtype=getattr(torch, dtype), device=keep.device)
            return out, C.c_void_p(out.data_ptr())
        out = np.empty(shape, getattr(np, dtype))
        return out, C.c_void_p(out.ctypes.data)

    def raycast(self, origins, directions, t_min=0.0, t_max=math.inf, bary=False):
        """The closest hit of each ray origins[i] + t directions[i] (n x ndim each, directions not normalised) with
        t_min <= t <= t_max: (t (n,) float32, primitives (n,) int64), with bary=True also the barycentrics (n, ndim - 1)
        float32.  No hit: +inf, -1, NaN; a ray with a non-finite origin or direction, or a zero direction: NaN, -1, NaN.
        Outputs live where the rays live (include/fi_hip.h fi_surface_raycast)."""
        o, d, mem, keep, n = self._rays(origins, directions)
        t, tp = self._like(keep[0], (n,), "float32")
        prim, pp = self._like(keep[0], (n,), "int64")
        b, bp = self._like(keep[0], (n, self.ndim - 1), "float32") if bary else (None, None)
        if n:   # (an empty tensor has no storage to point at)
            check(_capi.lib().fi_surface_raycast(self._h, n, o, d, float(t_min), float(t_max), tp, pp, bp, mem))
        return (t, prim, b) if bary else (t, prim)

    def count_hits(self, origins, directions, t_min=0.0, t_max=math.inf, limit=2**31 - 1):
        """The hits (n,) int32 of each ray with t_min <= t <= t_max, saturated at limit >= 1 (limit=1: is anything in the
        way); a ray that is none counts 0 (include/fi_hip.h fi_surface_count_hits)."""
        o, d, mem, keep, n = self._rays(origins, directions)
        c, cp = self._like(keep[0], (n,), "int32")
        if n:
            check(_capi.lib().fi_surface_count_hits(self._h, n, o, d, float(t_min), float(t_max), int(limit), cp, mem))
        return c

    def contains(self, points, direction=None):
        """bool (n,): the parity of the crossings of the ray from each point along `direction` (ndim values; None: +x).  A
        mesh that is not closed gives whatever the parity gives (include/fi_hip.h fi_surface_contains)."""
        p, mem, keep, n = self._rows("points", points)
        inside, ip = self._like(keep, (n,), "uint8")
        dv = None
        if direction is not None:
            dv = (C.c_float * self.ndim)(*[float(x) for x in np.asarray(direction, np.float64).reshape(self.ndim)])
        if n:
            check(_capi.lib().fi_surface_contains(self._h, n, p, dv, ip, mem))
        return inside.bool() if hasattr(inside, "data_ptr") else inside.astype(bool)

    def signed_distance(self, queries, max_distance=math.inf, primitives=False, closest=False):
        """SurfaceIndex.distance with the distances negated where contains(queries) holds along +x: negative inside a
        closed mesh, -0.0 on it, -inf inside and beyond max_distance (include/fi_hip.h fi_surface_signed_distance)."""
        q, mem, keep, n = self._rows("queries", queries)
        dist, dp = self._like(keep, (n,), "float32")
        idx, xp = self._like(keep, (n,), "int64") if primitives else (None, None)
        cl, cp = self._like(keep, (n, self.ndim), "float32") if closest else (None, None)
        if n:
            check(_capi.lib().fi_surface_signed_distance(self._h, n, q, float(max_distance), dp, xp, cp, mem))
        out = tuple(a for a in (dist, idx, cl) if a is not None)
        return out if len(out) > 1 else dist

    def signed_distance_field(self, sizes, max_distance=math.inf, primitives=False, device=False):
        """SurfaceIndex.signed_distance of every point of a lattice of `sizes` (x fastest), flat: numpy arrays, or torch
        tensors with device=True."""
        if len(sizes) != self.ndim:
            raise ValueError("sizes: %d extents for a %d-D surface" % (len(sizes), self.ndim))
        sz = (C.c_int * len(sizes))(*[int(s) for s in sizes])

        def call(d, i, mem):
            return _capi.lib().fi_surface_signed_distance_field(self._h, sz, float(max_distance), d, i, mem)
        return _distance_field(call, int(np.prod(sizes)), primitives, device)

    def render_depth(self, eye, target, up, fov_y, width, height):
        """A pinhole depth image of a 3-D surface: (t (height, width) float32, primitives (height, width) int64) of the
        rays from `eye` through the pixel centres, looking at `target` with `up` up and a vertical field of view of fov_y
        radians; row 0 is the top.  The directions have unit length, so t is the distance from the eye; +inf and -1 where
        nothing is hit."""
        if self.ndim != 3:
            raise ValueError("render_depth needs a 3-D surface")
        eye = np.asarray(eye, np.float64).reshape(3)
        fwd = np.asarray(target, np.float64).reshape(3) - eye
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, np.asarray(up, np.float64).reshape(3))
        right /= np.linalg.norm(right)
        top = np.cross(right, fwd)
        h = math.tan(0.5 * fov_y)
        x = ((np.arange(width) + 0.5) / width * 2 - 1) * h * width / height
        y = (1 - (np.arange(height) + 0.5) / height * 2) * h
        d = fwd[None, None, :] + x[None, :, None] * right[None, None, :] + y[:, None, None] * top[None, None, :]
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        d = d.reshape(-1, 3).astype(np.float32)
        o = np.broadcast_to(eye.astype(np.float32), d.shape)
        t, prim = self.raycast(o, d)
        return t.reshape(height, width), prim.reshape(height, width)


FI_SAMPLE_NORMALS = {"face": 0, "vertex": 1}


def _like_array(like, shape, dtype):
    """an uninitialised array of `shape`: a torch tensor on like's device when `like` is a CUDA tensor, else numpy
    -> (array, pointer or None for an empty one)"""
    if like is not None and like.is_cuda:
        import torch
        t = torch.empty(shape, dtype={np.float32: torch.float32, np.int64: torch.int64}[dtype], device=like.device)
        return t, (C.c_void_p(t.data_ptr()) if t.numel() else None)
    a = np.empty(shape, dtype)
    return a, (C.c_void_p(a.ctypes.data) if a.size else None)


def sample_mesh(mesh, n, seed=0, normals="face", primitives=False):
    """`n` points spread over `mesh` (an IsoMesh of numpy arrays, or of torch CUDA tensors; keys may be None) by area (2-D: by
    length) on the device: sample i lies in the i-th of n equal strata of the total area, placed by a counter-based hash of
    `seed`, so the points come out in ascending primitive order and a call is repeatable.  normals: "face" (the primitive's
    unit normal), "vertex" (the mesh's vertex normals interpolated and normalised; the mesh must have normals) or None;
    primitives=True: also the primitive each point lies on, int64.  Zero-area primitives are never sampled; a mesh with
    nothing to sample is refused (include/fi_hip.h fi_mesh_sample).  -> positions (n, ndim) float32, or a tuple (positions,
    normals, primitives) of what was asked for, where `mesh` lives"""
    if normals is not None and normals not in FI_SAMPLE_NORMALS:
        raise ValueError("normals is 'face', 'vertex' or None")
    n = int(n)
    if n < 0:
        raise ValueError("n must be >= 0")
    h, ndim, _mem, like = _mesh_handle(mesh)
    try:
        mem = FI_DEVICE if like is not None and like.is_cuda else FI_HOST
        pos, ppos = _like_array(like, (n, ndim), np.float32)
        nrm, pnrm = _like_array(like, (n, ndim), np.float32) if normals is not None else (None, None)
        prim, pprim = _like_array(like, (n,), np.int64) if primitives else (None, None)
        if n:
            check(_capi.lib().fi_mesh_sample(h, n, int(seed) & (2 ** 64 - 1), FI_SAMPLE_NORMALS[normals or "face"], ppos, pnrm, pprim, mem))
    finally:
        _capi.lib().fi_mesh_destroy(h)
    out = tuple(a for a in (pos, nrm, prim) if a is not None)
    return out if len(out) > 1 else pos


def _deviation_dict(r, ndim):
    return {"queries": int(r.queries), "counted": int(r.counted), "beyond": int(r.beyond), "invalid": int(r.invalid), "at": int(r.at),
            "max": float(r.max), "mean": float(r.mean), "rms": float(r.rms), "where": np.array(list(r.where)[:ndim], np.float32)}


def _deviation(h, surface, ndim, nv, like, samples, seed, max_distance, vertex_distances):
    """fi_mesh_deviation of a device mesh handle against a surface handle -> the dict of one direction"""
    of_s, of_v = _capi.FiDeviation(), _capi.FiDeviation()
    vd, pvd, mem = None, None, FI_HOST
    if vertex_distances:
        vd, pvd = _like_array(like, (nv,), np.float32)
        mem = FI_DEVICE if like is not None and like.is_cuda else FI_HOST
    check(_capi.lib().fi_mesh_deviation(h, surface, int(samples), int(seed) & (2 ** 64 - 1), float(max_distance), C.byref(of_s),
                                        C.byref(of_v), pvd, mem))
    out = {"samples": _deviation_dict(of_s, ndim), "vertices": _deviation_dict(of_v, ndim)}
    if vertex_distances:
        out["vertex_distances"] = vd
    return out


def mesh_deviation(a, b, samples=100_000, seed=0, max_distance=math.inf, symmetric=True, vertex_distances=False):
    """How far mesh `a` lies from surface `b`, measured on the device: the exact distances (SurfaceIndex.distance) of `samples`
    points spread over `a` (sample_mesh(a, samples, seed)) and of the vertices `a` uses, each list reduced to a dict of
    queries, counted, beyond (further than max_distance), invalid (a non-finite vertex), max, mean, rms, at (the first query
    holding max; -1 when nothing is counted) and where (its position) -- the same bytes on every run.  `a` and `b` are
    IsoMeshes of numpy arrays or of torch CUDA tensors; `b` may also be a SurfaceIndex, which holds no mesh: symmetric=True
    then raises ValueError.  vertex_distances=True adds the distance of every vertex (NaN for an unused one), where the mesh
    lives.  -> {"a_to_b": {"samples": ..., "vertices": ...[, "vertex_distances": ...]}, "b_to_a": the same the other way or
    None, "hausdorff": the largest max of all} (include/fi_hip.h fi_mesh_deviation)"""
    if int(samples) < 0:
        raise ValueError("samples must be >= 0")
    L = _capi.lib()
    given = isinstance(b, SurfaceIndex)
    if given and symmetric:
        raise ValueError("symmetric=True needs b as a mesh: a SurfaceIndex holds no mesh to sample")
    ha, ndim, _mem, like_a = _mesh_handle(a)
    hb, sa, sb = None, C.c_void_p(), C.c_void_p()
    try:
        if given:
            if b.ndim != ndim:
                raise ValueError("a is %d-D, b is %d-D" % (ndim, b.ndim))
            surface = b._h
        else:
            hb, ndim_b, _mem, like_b = _mesh_handle(b)
            if ndim_b != ndim:
                raise ValueError("a is %d-D, b is %d-D" % (ndim, ndim_b))
            check(L.fi_surface_from_mesh(C.byref(sb), hb))
            surface = sb
        out = {"a_to_b": _deviation(ha, surface, ndim, int(a.vertices.shape[0]), like_a, samples, seed, max_distance, vertex_distances),
               "b_to_a": None}
        if symmetric:
            check(L.fi_surface_from_mesh(C.byref(sa), ha))
            out["b_to_a"] = _deviation(hb, sa, ndim, int(b.vertices.shape[0]), like_b, samples, seed, max_distance, vertex_distances)
    finally:
        for s in (sa, sb):
            if s:
                L.fi_surface_destroy(s)
        for h in (ha, hb):
            if h:
                L.fi_mesh_destroy(h)
    out["hausdorff"] = max(d[k]["max"] for d in (out["a_to_b"], out["b_to_a"]) if d is not None for k in ("samples", "vertices"))
    return out


def _register_options(mode, max_iterations, max_distance, rotation_tolerance, translation_tolerance, loss, scale, tuning):
    if mode not in _capi.FI_REGISTER:
        raise ValueError("mode is 'plane' or 'point', not %r" % (mode,))
    if loss is not None and loss not in _capi.FI_LOSS:
        raise ValueError("loss is None, 'huber', 'cauchy' or 'tukey', not %r" % (loss,))
    return _capi.FiRegisterOptions(_capi.FI_REGISTER[mode], int(max_iterations), float(max_distance), float(rotation_tolerance),
                                   float(translation_tolerance), _capi.FI_LOSS_NONE if loss is None else _capi.FI_LOSS[loss],
                                   float(tuning), float(scale))


def _register(call, ndim, source, opt, initial, transformed, distances, other_memory=()):
    """Shared body of the registrations: call(n, source, options, initial, result, transformed, distances, memory) -> the dict"""
    s, smem, skeep = _buf(source)
    shape = tuple(skeep.shape)
    if len(shape) != 2 or shape[1] != ndim:
        raise ValueError("source is (n, %d) for a %d-D target, not %r" % (ndim, ndim, shape))
    mem = _same_memory(smem, *other_memory)
    n = int(shape[0])
    init = None
    if initial is not None:
        init = np.ascontiguousarray(initial, np.float64)
        if init.shape != (ndim + 1, ndim + 1):
            raise ValueError("initial is a (%d, %d) matrix" % (ndim + 1, ndim + 1))
    like = skeep if hasattr(skeep, "data_ptr") else None
    moved, pmoved = _like_array(like, (n, ndim), np.float32) if transformed else (None, None)
    dist, pdist = _like_array(like, (n,), np.float32) if distances else (None, None)
    r = _capi.FiRegistration()
    check(call(n, s if n else None, C.byref(opt), None if init is None else init.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r),
               pmoved, pdist, mem))
    out = {"transform": np.array(list(r.transform)[:(ndim + 1) ** 2], np.float64).reshape(ndim + 1, ndim + 1)}
    for k in ("iterations", "converged", "fixed_mask", "queries", "counted", "beyond", "invalid", "degenerate"):
        out[k] = int(getattr(r, k))
    for k in ("rms", "weighted_rms", "last_rotation", "last_translation"):
        out[k] = float(getattr(r, k))
    if transformed:
        out["transformed"] = moved
    if distances:
        out["distances"] = dist
    return out


def _register_to_mesh(h, surface, ndim, source, opt, initial, transformed, distances, other_memory=()):
    def call(n, s, o, init, r, moved, dist, mem):
        return _capi.lib().fi_mesh_register(h, surface, n, s, o, init, r, moved, dist, mem)
    return _register(call, ndim, source, opt, initial, transformed, distances, other_memory)


def register_points(source, target, target_normals=None, mode="plane", max_iterations=30, max_distance=math.inf,
                    rotation_tolerance=1e-6, translation_tolerance=1e-6, loss=None, scale=0.0, tuning=0.0, initial=None,
                    transformed=False, distances=False):
    """The rigid transform that lays the points `source` (n, ndim) over `target` by iterated closest points on the device,
    2-D or 3-D.  target: an IsoMesh (its exact closest points), a PointIndex or an (m, ndim) array of points (their nearest
    point) -- numpy arrays, or torch CUDA tensors in the same memory as `source`; a bare SurfaceIndex holds no vertices to
    take normals from and is accepted with mode="point" only (ValueError otherwise).  mode="plane" minimises the distances
    along the target's normals (a mesh's face normals; a point set needs target_normals (m, ndim)) and converges in a few
    steps; mode="point" minimises the distances themselves.  Pairs further apart than max_distance are left out; loss
    ("huber", "cauchy", "tukey" with a residual `scale` > 0 and an optional `tuning` constant) weighs outliers down.  The loop
    stops when a step turns by at most rotation_tolerance (radians) and shifts by at most translation_tolerance, or after
    max_iterations steps; initial: a (ndim + 1, ndim + 1) matrix to start from (coarse alignment is the caller's).
    -> a dict: transform (ndim + 1, ndim + 1) float64 mapping source to target coordinates, iterations, converged, fixed_mask
    (the unknowns the data could not see, e.g. a plane's slide), queries, counted, beyond, invalid, degenerate, rms,
    weighted_rms, last_rotation, last_translation, and with transformed / distances the moved points and their last
    distances where `source` lives (include/fi_hip.h fi_mesh_register)."""
    opt = _register_options(mode, max_iterations, max_distance, rotation_tolerance, translation_tolerance, loss, scale, tuning)
    L = _capi.lib()
    if isinstance(target, SurfaceIndex):
        if mode != "point":
            raise ValueError("mode='plane' needs the target as a mesh: a SurfaceIndex holds no vertices to take normals from")
        return _register_to_mesh(None, target._h, target.ndim, source, opt, initial, transformed, distances)
    if isinstance(target, IsoMesh):
        h, ndim, mem, _like = _mesh_handle(target)
        try:
            return _register_to_mesh(h, None, ndim, source, opt, initial, transformed, distances, [mem])
        finally:
            L.fi_mesh_destroy(h)
    index, memory = target, []
    if not isinstance(target, PointIndex):
        memory = [_buf(target)[1]]
        index = PointIndex(target)
    tn, tmem, tkeep = _buf(target_normals)
    if mode == "plane" and tn is None:
        raise ValueError("mode='plane' on a point set needs target_normals")
    if tn is not None and tuple(tkeep.shape) != (index.num_points, index.ndim):
        raise ValueError("target_normals is (%d, %d), one per target point" % (index.num_points, index.ndim))

    def call(n, s, o, init, r, moved, dist, mem):
        return L.fi_points_register(index._h, tn, n, s, o, init, r, moved, dist, mem)
    return _register(call, index.ndim, source, opt, initial, transformed, distances, memory + [tmem])


def apply_transform(transform, points, normals=None):
    """`points` (n, ndim) moved by a register_points transform, R x + t in float64, and with `normals` also R n -- numpy in,
    numpy out; torch in, torch out.  A convenience: register_points' own `transformed` follows the contract's rounding (one
    fp32 rounding of a fixed-order sum), this does not."""
    if hasattr(points, "data_ptr"):
        import torch
        T = torch.as_tensor(np.asarray(transform, np.float64), device=points.device)
        D = T.shape[0] - 1
        moved = points.to(torch.float64) @ T[:D, :D].T + T[:D, D]
        return moved if normals is None else (moved, normals.to(torch.float64) @ T[:D, :D].T)
    T = np.asarray(transform, np.float64)
    D = T.shape[0] - 1
    moved = np.asarray(points, np.float64) @ T[:D, :D].T + T[:D, D]
    return moved if normals is None else (moved, np.asarray(normals, np.float64) @ T[:D, :D].T)


def _rows(a):
    return int(a.shape[0])


def thin_points(positions, cell, normals=None, values=None, origin=None, mode="mean", counts=False, indices=False, cell_map=False):
    """A point cloud thinned on a uniform grid of spacing `cell` on the device: one output point per occupied cell, in
    ascending cell order.  positions (n, ndim) -- or (n,) in 1-D -- with optional normals (n, ndim) and values (n,), numpy
    arrays or torch CUDA tensors (all in the same memory).  mode="mean": the members' mean position and value and their
    summed, normalised normal; mode="first": the member with the lowest index, bit for bit.  origin: where cell (0, ..) starts
    (default zeros).  Non-finite points are left out.  counts / indices / cell_map=True add each cell's number of members
    (int32), its lowest member's index (int64) and, per input point, the output it went to (int32, -1 for a point left out).
    -> positions, or a tuple (positions, normals, values, counts, indices, cell_map) of what was given and asked for, where
    `positions` lives (include/fi_hip.h fi_cloud_thin)."""
    if mode not in _capi.FI_THIN:
        raise ValueError("mode is 'mean' or 'first', not %r" % (mode,))
    p, pmem, pkeep = _buf(positions)
    shape = tuple(pkeep.shape)
    if len(shape) not in (1, 2):
        raise ValueError("positions is (n, ndim), or (n,) in 1-D, not %r" % (shape,))
    n, ndim = shape[0], (shape[1] if len(shape) == 2 else 1)
    nr, nmem, nkeep = _buf(normals)
    if normals is not None and tuple(nkeep.shape) != shape:
        raise ValueError("normals is %r, one per point" % (shape,))
    vl, vmem, vkeep = _buf(values)
    if values is not None and tuple(vkeep.shape) != (n,):
        raise ValueError("values is (%d,), one per point" % n)
    mem = _same_memory(pmem, nmem, vmem)
    o = None
    if origin is not None:
        o = np.ascontiguousarray(origin, np.float32).reshape(-1)
        if o.size != ndim:
            raise ValueError("origin has %d coordinates" % ndim)
    dev = pkeep.device if mem == FI_DEVICE else None
    out = [_cloud_out(dev, shape, np.float32),
           _cloud_out(dev, shape, np.float32) if normals is not None else None,
           _cloud_out(dev, (n,), np.float32) if values is not None else None,
           _cloud_out(dev, (n,), np.int32) if counts else None,
           _cloud_out(dev, (n,), np.int64) if indices else None,
           _cloud_out(dev, (n,), np.int32) if cell_map else None]
    ptr = [None if a is None else a[1] for a in out]
    num = C.c_long(0)
    check(_capi.lib().fi_cloud_thin(ndim, n, p if n else None, nr, vl, float(cell),
                                    None if o is None else o.ctypes.data_as(C.POINTER(C.c_float)), _capi.FI_THIN[mode], *ptr,
                                    C.byref(num), mem))
    m = num.value
    trim = lambda a: a[:m].clone() if hasattr(a, "data_ptr") else a[:m].copy()  # noqa: E731
    got = tuple(a[0] if i == 5 else trim(a[0]) for i, a in enumerate(out) if a is not None)
    return got if len(got) > 1 else got[0]


def _flags(a):
    """(pointer, memory kind, keep-alive object) of a mask as uint8 flags: a numpy array, a torch tensor, or None"""
    if a is None:
        return None, None, None
    if hasattr(a, "data_ptr"):
        import torch
        t = a.to(torch.uint8).contiguous()
        return C.c_void_p(t.data_ptr()), (FI_DEVICE if t.is_cuda else FI_HOST), t
    arr = np.ascontiguousarray(a).astype(np.uint8)
    return C.c_void_p(arr.ctypes.data), FI_HOST, arr


def _plane_options(ndim, threshold, max_trials, confidence, refine, seed, axis, max_angle):
    opt = _capi.FiPlaneOptions(float(threshold), int(max_trials), float(confidence), int(refine), int(seed) & (2 ** 64 - 1))
    if (axis is None) != (max_angle is None):
        raise ValueError("axis and max_angle go together")
    if axis is not None:
        ax = np.ascontiguousarray(axis, np.float32).reshape(-1)
        if ax.size != ndim:
            raise ValueError("axis has %d coordinates" % ndim)
        if not 0.0 <= float(max_angle) <= 90.0:
            raise ValueError("max_angle is in degrees, 0 .. 90")
        opt.axis[:ndim] = ax.tolist()
        opt.min_cos = float(np.float32(math.cos(math.radians(float(max_angle)))))   # no trigonometry on the device
    return opt


def _plane_dict(m, ndim):
    return {"found": bool(m.found), "normal": np.array(m.normal[:ndim], np.float64), "offset": float(m.offset),
            "inliers": int(m.inliers), "candidates": int(m.candidates), "trials": int(m.trials), "refits": int(m.refits),
            "rms": float(m.rms)}


def _plane_cloud(positions, mask):
    p, pmem, pkeep = _buf(positions)
    shape = tuple(pkeep.shape)
    if len(shape) != 2:
        raise ValueError("positions is (n, ndim), not %r" % (shape,))
    mk, mmem, mkeep = _flags(mask)
    if mask is not None and tuple(mkeep.shape) != (shape[0],):
        raise ValueError("mask is (%d,), one per point" % shape[0])
    return p, mk, shape[0], shape[1], _same_memory(pmem, mmem), (pkeep, mkeep)


def segment_plane(positions, threshold, max_trials=1024, confidence=0.999, refine=2, seed=0, mask=None, axis=None, max_angle=None):
    """The dominant plane (3-D) or line (2-D) of a point cloud on the device: RANSAC with an exact inlier count, then
    `refine` least-squares refits.  positions (n, ndim), a numpy array or a torch CUDA tensor that stays on the device; a point
    within `threshold` of the plane (inclusive) is an inlier.  At most max_trials hypotheses, fewer once the best one would
    have been drawn with probability `confidence` (0: never stop early); mask (n,): the points that take part; axis and
    max_angle (degrees): only planes whose normal lies within that angle of +-axis.  -> (model, inliers): a dict with `found`,
    `normal` (float64 (ndim,), its largest component positive), `offset` (normal . x + offset = 0), `inliers`, `candidates`,
    `trials`, `refits` and `rms`, and a boolean mask (n,) where `positions` lives.  Every figure is defined bit for bit
    (include/fi_hip.h fi_plane_fit)."""
    p, mk, n, ndim, mem, keep = _plane_cloud(positions, mask)
    opt = _plane_options(ndim, threshold, max_trials, confidence, refine, seed, axis, max_angle)
    model = _capi.FiPlaneModel()
    out, ptr = _cloud_out(keep[0].device if mem == FI_DEVICE else None, (n,), np.uint8)
    check(_capi.lib().fi_plane_fit(ndim, n, p if n else None, mk if n else None, C.byref(opt), C.byref(model), ptr, mem))
    return _plane_dict(model, ndim), _as_mask(out)


def segment_planes(positions, threshold, max_planes, min_inliers=0, max_trials=1024, confidence=0.999, refine=2, seed=0, mask=None,
                   axis=None, max_angle=None):
    """Up to max_planes planes (3-D) or lines (2-D) peeled off a point cloud on the device, one after the other: plane p is
    segment_plane with seed + p over the points no earlier plane took; the loop ends at the first plane with fewer than
    min_inliers inliers, which is not recorded.  -> (labels, models): labels (n,) int32 where `positions` lives, the plane that
    took each point or -1, and the list of segment_plane's model dicts (include/fi_hip.h fi_planes_segment)."""
    p, mk, n, ndim, mem, keep = _plane_cloud(positions, mask)
    opt = _plane_options(ndim, threshold, max_trials, confidence, refine, seed, axis, max_angle)
    rows = (_capi.FiPlaneModel * max(int(max_planes), 1))()
    found = C.c_int(0)
    labels, ptr = _cloud_out(keep[0].device if mem == FI_DEVICE else None, (n,), np.int32)
    check(_capi.lib().fi_planes_segment(ndim, n, p if n else None, mk if n else None, C.byref(opt), int(max_planes), int(min_inliers),
                                        ptr, rows, C.byref(found), mem))
    return labels, [_plane_dict(rows[i], ndim) for i in range(found.value)]


def _shape_options(kind, threshold, r_min, r_max, has_normals, max_angle, max_trials, confidence, refine, seed):
    if kind not in _capi.FI_SHAPE:
        raise ValueError("kind is 'sphere' or 'cylinder', not %r" % (kind,))
    normal_cos = 0.0
    if max_angle is not None:
        if not has_normals:
            raise ValueError("max_angle needs normals")
        if not 0.0 <= float(max_angle) < 90.0:
            raise ValueError("max_angle is in degrees, 0 .. 90 (90 excluded: leave it out)")
        normal_cos = float(np.float32(math.cos(math.radians(float(max_angle)))))   # no trigonometry on the device
    return _capi.FiShapeOptions(_capi.FI_SHAPE[kind], float(threshold), float(r_min), float(r_max), normal_cos, int(max_trials),
                                float(confidence), int(refine), int(seed) & (2 ** 64 - 1))


def _shape_dict(m, ndim, kind):
    out = {"found": bool(m.found), "kind": kind,
           "center": np.array(m.center[:ndim], np.float64), "radius": float(m.radius), "inliers": int(m.inliers),
           "candidates": int(m.candidates), "trials": int(m.trials), "refits": int(m.refits), "rms": float(m.rms)}
    if kind == "cylinder":
        out["axis"] = np.array(m.axis[:], np.float64)
        out["extent"] = np.array(m.extent[:], np.float64)
    return out


def _shape_cloud(positions, normals, mask):
    p, mk, n, ndim, mem, keep = _plane_cloud(positions, mask)
    nr, nmem, nkeep = _buf(normals)
    if normals is not None and tuple(nkeep.shape) != (n, ndim):
        raise ValueError("normals is (%d, %d), one per point" % (n, ndim))
    return p, nr, mk, n, ndim, _same_memory(mem, nmem), keep + (nkeep,)


def _segment_shape(kind, positions, normals, threshold, r_min, r_max, max_angle, max_trials, confidence, refine, seed, mask):
    p, nr, mk, n, ndim, mem, keep = _shape_cloud(positions, normals, mask)
    opt = _shape_options(kind, threshold, r_min, r_max, normals is not None, max_angle, max_trials, confidence, refine, seed)
    model = _capi.FiShapeModel()
    out, ptr = _cloud_out(keep[0].device if mem == FI_DEVICE else None, (n,), np.uint8)
    check(_capi.lib().fi_shape_fit(ndim, n, p if n else None, nr if n else None, mk if n else None, C.byref(opt), C.byref(model), ptr, mem))
    return _shape_dict(model, ndim, kind), _as_mask(out)


def segment_sphere(positions, threshold, r_min=0.0, r_max=math.inf, normals=None, max_angle=None, max_trials=1024, confidence=0.999,
                   refine=2, seed=0, mask=None):
    """The dominant sphere (3-D) or circle (2-D) of a point cloud on the device: RANSAC with an exact inlier count, then
    `refine` algebraic least-squares refits.  positions (n, ndim), a numpy array or a torch CUDA tensor that stays on the device;
    a point whose distance from the sphere is within `threshold` (inclusive) is an inlier.  Only radii in [r_min, r_max] are
    considered.  normals (n, ndim), optional: points without a usable normal take no part, and with max_angle (degrees) an
    inlier's normal must also lie within that angle of the sphere's, either way round.  At most max_trials hypotheses, fewer
    once the best one would have been drawn with probability `confidence` (0: never stop early); mask (n,): the points that
    take part.  -> (model, inliers): a dict with `found`, `kind`, `center` (float64 (ndim,)), `radius`, `inliers`, `candidates`,
    `trials`, `refits` and `rms`, and a boolean mask (n,) where `positions` lives.  Every figure is defined bit for bit
    (include/fi_hip.h fi_shape_fit)."""
    return _segment_shape("sphere", positions, normals, threshold, r_min, r_max, max_angle, max_trials, confidence, refine, seed, mask)


def segment_cylinder(positions, normals, threshold, r_min=0.0, r_max=math.inf, max_angle=None, max_trials=1024, confidence=0.999,
                     refine=2, seed=0, mask=None):
    """The dominant cylinder of a 3-D point cloud with normals on the device: two points and their normals make a hypothesis
    (the axis across both normals, through the point the two normal lines come closest at), scored and refitted as
    segment_sphere's.  -> (model, inliers): segment_sphere's dict with `kind` 'cylinder', `center` a point of the axis, and two
    more entries: `axis` (float64 (3,), its largest component positive) and `extent`, the least and the greatest
    (x - center) . axis over the inliers (include/fi_hip.h fi_shape_fit)."""
    if normals is None:
        raise ValueError("a cylinder needs normals")
    return _segment_shape("cylinder", positions, normals, threshold, r_min, r_max, max_angle, max_trials, confidence, refine, seed, mask)


def segment_shapes(positions, kind, threshold, max_shapes, min_inliers=0, normals=None, r_min=0.0, r_max=math.inf, max_angle=None,
                   max_trials=1024, confidence=0.999, refine=2, seed=0, mask=None):
    """Up to max_shapes shapes of one `kind` ('sphere' or 'cylinder') peeled off a point cloud on the device, one after the
    other: shape p is segment_sphere / segment_cylinder with seed + p over the points no earlier shape took; the loop ends at
    the first shape with fewer than min_inliers inliers, which is not recorded.  -> (labels, models): labels (n,) int32 where
    `positions` lives, the shape that took each point or -1, and the list of model dicts (include/fi_hip.h
    fi_shapes_segment)."""
    p, nr, mk, n, ndim, mem, keep = _shape_cloud(positions, normals, mask)
    opt = _shape_options(kind, threshold, r_min, r_max, normals is not None, max_angle, max_trials, confidence, refine, seed)
    rows = (_capi.FiShapeModel * max(int(max_shapes), 1))()
    found = C.c_int(0)
    labels, ptr = _cloud_out(keep[0].device if mem == FI_DEVICE else None, (n,), np.int32)
    check(_capi.lib().fi_shapes_segment(ndim, n, p if n else None, nr if n else None, mk if n else None, C.byref(opt), int(max_shapes),
                                        int(min_inliers), ptr, rows, C.byref(found), mem))
    return labels, [_shape_dict(rows[i], ndim, kind) for i in range(found.value)]


def _match(a, b, valid_a, valid_b, distances):
    pa, amem, akeep = _buf(a)
    pb, bmem, bkeep = _buf(b)
    if len(akeep.shape) != 2 or len(bkeep.shape) != 2 or akeep.shape[1] != bkeep.shape[1]:
        raise ValueError("a is (n_a, dim) and b is (n_b, dim), not %r and %r" % (tuple(akeep.shape), tuple(bkeep.shape)))
    na, nb, dim = int(akeep.shape[0]), int(bkeep.shape[0]), int(akeep.shape[1])
    va, vamem, vakeep = _flags(valid_a)
    vb, vbmem, vbkeep = _flags(valid_b)
    for mask, n in ((vakeep, na), (vbkeep, nb)):
        if mask is not None and tuple(mask.shape) != (n,):
            raise ValueError("a mask is (%d,), one per row" % n)
    mem = _same_memory(amem, bmem, vamem, vbmem)
    dev = akeep.device if mem == FI_DEVICE else None
    idx, pi = _cloud_out(dev, (na,), np.int64)
    dist, pd = _cloud_out(dev, (na,), np.float32) if distances else (None, None)
    check(_capi.lib().fi_feature_match(dim, na, pa if na else None, va if na else None, nb, pb if nb else None, vb if nb else None,
                                       pi, pd, mem))
    return idx, dist


def match_features(a, b, valid_a=None, valid_b=None, mutual=False, distances=False):
    """For every row of `a` (n_a, dim) the nearest row of `b` (n_b, dim) on the device, 1 <= dim <= 64: the squared distance is
    summed in fp32 over ascending columns, equal distances go to the smallest index, and only rows that are finite and not
    masked out (valid_a, valid_b: one flag a row) take part.  -> indices (n_a,) int64, -1 for a row without a match, and with
    distances=True also the distances (n_a,) float32, +inf there.  mutual=True runs the match both ways and keeps i -> j only
    where j's own match is i.  numpy arrays, or torch CUDA tensors that stay on the device, all in the same memory
    (include/fi_hip.h fi_feature_match)."""
    idx, dist = _match(a, b, valid_a, valid_b, distances)
    if mutual:
        back, _ = _match(b, a, valid_b, valid_a, False)
        if hasattr(idx, "data_ptr"):
            import torch
            here = torch.arange(idx.shape[0], device=idx.device)
            lost = (idx >= 0) & ((back[idx.clamp(min=0)] != here) if back.shape[0] else torch.zeros_like(idx, dtype=torch.bool))
        else:
            lost = (idx >= 0) & ((back[np.maximum(idx, 0)] != np.arange(len(idx))) if len(back) else np.zeros(len(idx), bool))
        idx[lost] = -1
        if dist is not None:
            dist[lost] = math.inf
    return (idx, dist) if distances else idx


def _alignment_dict(r):
    return {"found": bool(r.found), "transform": np.array(r.transform[:], np.float64).reshape(4, 4), "inliers": int(r.inliers),
            "pairs": int(r.pairs), "live": int(r.live), "trials": int(r.trials), "valid": int(r.valid), "rms": float(r.rms)}


def align_correspondences(source, target, src_index, tgt_index, threshold, similarity=0.9, max_trials=100_000, confidence=0.999,
                          seed=0):
    """The rotation and shift that carries the most of the matched pairs (source[src_index[c]], target[tgt_index[c]]) to within
    `threshold` of each other, by RANSAC on the device: the coarse alignment from any pose.  source (n_s, 3), target (n_t, 3),
    the indices (m,) int64 -- numpy arrays, or torch CUDA tensors that stay on the device, all in the same memory.  A
    hypothesis is three pairs; it is refused where an edge of its source triangle and the same edge of its target triangle
    differ by more than the factor `similarity` (0: no such test), which spares scoring most wrong ones.  At most max_trials
    hypotheses, fewer once the best would have been drawn with probability `confidence` (0: never stop early).  A pair with
    an index out of range (-1, say, for no match) or a non-finite point takes no part.  -> (result, inliers): a dict with
    `found`, `transform` (4, 4) float64 mapping source to target coordinates -- register_points' `initial` --, `inliers`,
    `pairs`, `live`, `trials`, `valid` (the hypotheses that were scored) and `rms`, and a boolean mask (m,) where the inputs
    live.  Every figure is defined bit for bit (include/fi_hip.h fi_align_correspondences)."""
    ps, smem, skeep = _buf(source)
    pt, tmem, tkeep = _buf(target)
    for what, keep in (("source", skeep), ("target", tkeep)):
        if len(keep.shape) != 2 or keep.shape[1] != 3:
            raise ValueError("%s is (n, 3), not %r" % (what, tuple(keep.shape)))
    pi, imem, ikeep = _buf(src_index, np.int64)
    pj, jmem, jkeep = _buf(tgt_index, np.int64)
    if len(ikeep.shape) != 1 or tuple(ikeep.shape) != tuple(jkeep.shape):
        raise ValueError("src_index and tgt_index are (m,) each, not %r and %r" % (tuple(ikeep.shape), tuple(jkeep.shape)))
    ns, nt, m = int(skeep.shape[0]), int(tkeep.shape[0]), int(ikeep.shape[0])
    mem = _same_memory(smem, tmem, imem, jmem)
    opt = _capi.FiAlignOptions(float(threshold), float(similarity), int(max_trials), float(confidence), int(seed) & (2 ** 64 - 1))
    res = _capi.FiAlignment()
    out, ptr = _cloud_out(skeep.device if mem == FI_DEVICE else None, (m,), np.uint8)
    check(_capi.lib().fi_align_correspondences(ns, ps if ns else None, nt, pt if nt else None, m, pi if m else None,
                                               pj if m else None, C.byref(opt), C.byref(res), ptr, mem))
    return _alignment_dict(res), _as_mask(out)


_ALIGN_KEYWORDS = ("similarity", "max_trials", "confidence", "seed")


def register_global(source, source_normals, target, target_normals, threshold, k=32, mutual=False, refine=True, **keywords):
    """`source` (n, 3) laid over `target` (m, 3) from any pose, on the device: both clouds described (PointIndex.describe over k
    neighbours and the normals), every source descriptor matched to its nearest target descriptor (match_features; mutual as
    there), the motion most matches agree on to within `threshold` (align_correspondences), and with refine=True that motion
    handed as `initial` to register_points(source, target, target_normals=..., max_distance=3 * threshold).  keywords:
    align_correspondences' similarity, max_trials, confidence and seed; any other goes to register_points.  numpy arrays, or
    torch CUDA tensors that stay on the device.  -> (alignment, registration): align_correspondences' dict with `matches`
    (n,), the target point of every source point or -1, and `mask` (n,), the matches the motion keeps; and register_points'
    dict, or None without refine."""
    align_kw = {key: keywords.pop(key) for key in _ALIGN_KEYWORDS if key in keywords}
    on_device = bool(getattr(source, "is_cuda", False))
    fs, vs = PointIndex(source).describe(source_normals, k, device=on_device)
    target_index = PointIndex(target)
    ft, vt = target_index.describe(target_normals, k, device=on_device)
    matches = match_features(fs, ft, vs, vt, mutual=mutual)
    if on_device:
        import torch
        here = torch.arange(matches.shape[0], device=matches.device)
    else:
        here = np.arange(len(matches), dtype=np.int64)
    alignment, mask = align_correspondences(source, target, here, matches, threshold, **align_kw)
    alignment["matches"], alignment["mask"] = matches, mask
    if not refine:
        return alignment, None
    keywords.setdefault("max_distance", 3.0 * float(threshold))
    return alignment, register_points(source, target_index, target_normals=target_normals, initial=alignment["transform"], **keywords)


def smooth_points(positions, radius, k=32, degree=2, max_move=math.inf, normals=None, curvature=False, order=False):
    """PointIndex(positions).smooth(...): the cloud's points moved onto the local surface of their neighbours, with its normals
    -- what reduces the measurement noise of a scan before estimate_normals / sdf_from_points.  numpy arrays, or torch CUDA
    tensors that stay on the device."""
    return PointIndex(positions).smooth(k=k, radius=radius, degree=degree, max_move=max_move, normals=normals, curvature=curvature,
                                        order=order, device=bool(getattr(positions, "is_cuda", False)))


def clean_points(positions, normals=None, values=None, cell=None, k=None, std_ratio=2.0, radius=None, min_neighbours=2,
                 max_distance=math.inf, cluster_eps=None, cluster_min_points=1, largest=None, min_cluster=0, remove_planes=None,
                 smooth=None):
    """A scan made fit for estimate_normals / sdf_from_points on the device, in this order and each step only if asked for:
    thin_points(cell) (mean mode), PointIndex.radius_outliers(radius, min_neighbours), PointIndex.statistical_outliers(k,
    std_ratio, max_distance).  Each filter builds its PointIndex over what the step before left.  numpy arrays, or torch
    CUDA tensors that stay on the device.  -> (positions, normals, values, report): the surviving arrays (None where none was
    given) and a dict with `input`, `output`, what each stage removed (`thinned`, `radius`, `statistical`) and the
    statistical stage's `stats`.  With cluster_eps a last step runs after the outlier rules, for the stray CLUMP that both of
    them keep: PointIndex.cluster(cluster_eps, cluster_min_points) over what is left, and only the points of the clusters
    that keep_clusters(rows, largest, min_cluster) chooses survive (noise points go); the report gains `cluster`, what the
    step removed, and `clusters`, its stats.  remove_planes, a dict of segment_planes' arguments (threshold and max_planes at
    least), takes the floor or table a scan stands on out after the outlier rules and BEFORE the cluster step -- an object
    touches what it stands on, so clustering alone cannot part them: the points segment_planes labels go, and the report
    gains `planes`, what the step removed, and `plane_models`, the models.  smooth, a dict of smooth_points' arguments (radius
    at least), runs as the very last step on the points that are kept: their positions become smooth_points(positions,
    normals=the kept normals, **smooth)'s, the normals (if any were given) the fitted surface's with the given normals' sign,
    and the report gains `smoothed`, how many points were fitted (order >= 1), and `smooth_order`, each point's order."""
    as_array = lambda a: a if a is None or hasattr(a, "data_ptr") else np.ascontiguousarray(a, np.float32)  # noqa: E731
    pos, nrm, val = as_array(positions), as_array(normals), as_array(values)
    on_device = bool(getattr(pos, "is_cuda", False))
    report = {"input": _rows(pos)}

    def select(keep):
        return tuple(a if a is None else a[keep] for a in (pos, nrm, val))
    if cell is not None:
        got = thin_points(pos, cell, nrm, val)
        got = iter(got if isinstance(got, tuple) else (got,))
        before = _rows(pos)
        pos = next(got)
        nrm = next(got) if nrm is not None else None
        val = next(got) if val is not None else None
        report["thinned"] = before - _rows(pos)
    if radius is not None:
        keep, kept = PointIndex(pos).radius_outliers(radius, min_neighbours, device=on_device)
        report["radius"] = _rows(pos) - kept
        pos, nrm, val = select(keep)
    if k is not None:
        keep, stats = PointIndex(pos).statistical_outliers(k, std_ratio, max_distance, device=on_device)
        report["statistical"] = _rows(pos) - stats["kept"]
        report["stats"] = stats
        pos, nrm, val = select(keep)
    if remove_planes is not None:
        labels, models = segment_planes(pos, **remove_planes)
        keep = labels < 0
        report["planes"] = _rows(pos) - int(keep.sum())
        report["plane_models"] = models
        pos, nrm, val = select(keep)
    if cluster_eps is not None:
        labels, stats = PointIndex(pos).cluster(cluster_eps, cluster_min_points, stats=True, device=on_device)
        chosen = keep_clusters(cluster_measure(pos, labels, num_clusters=stats["clusters"]), largest, min_cluster)
        chosen = np.concatenate([chosen, [False]])           # (the label -1 reads the entry at the end)
        if on_device:
            import torch
            keep = torch.from_numpy(chosen).to(labels.device)[labels.long()]
        else:
            keep = chosen[labels]
        report["cluster"] = _rows(pos) - int(keep.sum())
        report["clusters"] = stats
        pos, nrm, val = select(keep)
    if smooth is not None:
        args = dict(smooth)
        args.pop("order", None)
        args.pop("normals", None)
        got = smooth_points(pos, normals=nrm, order=True, **args)
        pos = got[0]
        nrm = got[1] if nrm is not None else None
        report["smooth_order"] = got[-1]
        report["smoothed"] = int((got[-1] > 0).sum())
    report["output"] = _rows(pos)
    return pos, nrm, val, report


def cluster_points(positions, eps, min_points=1, measure=False):
    """The clusters of a point cloud on the device: PointIndex(positions).cluster(eps, min_points) -> labels (n,) int32,
    where `positions` lives (numpy, or a torch CUDA tensor); measure=True: -> (labels, rows), rows being cluster_measure's
    table of the clusters found."""
    on_device = bool(getattr(positions, "is_cuda", False))
    labels, stats = PointIndex(positions).cluster(eps, min_points, stats=True, device=on_device)
    if not measure:
        return labels
    return labels, cluster_measure(positions, labels, num_clusters=stats["clusters"])


def cluster_measure(positions, labels, core=None, num_clusters=None):
    """One row per cluster of a labelling of `positions` (n, ndim) -- or (n,) in 1-D -- by `labels` (n,) int32 with values in
    [-1, num_clusters) (default: the largest label + 1), found on the device: a list of dicts with `count`, `core` (the
    members flagged in the mask `core`, 0 without one), `lo` / `hi` (the bounding box, float32 (ndim,)) and `centroid`
    (float64 (ndim,), summed in a fixed order).  numpy arrays or torch CUDA tensors, all in the same memory (include/fi_hip.h
    fi_cluster_measure)."""
    p, pmem, pkeep = _buf(positions)
    shape = tuple(pkeep.shape)
    if len(shape) not in (1, 2):
        raise ValueError("positions is (n, ndim), or (n,) in 1-D, not %r" % (shape,))
    n, ndim = shape[0], (shape[1] if len(shape) == 2 else 1)
    lb, lmem, lkeep = _buf(labels, np.int32)
    if tuple(lkeep.shape) != (n,):
        raise ValueError("labels is (%d,), one per point" % n)
    cr, cmem, ckeep = None, None, None
    if core is not None:
        if hasattr(core, "data_ptr"):
            import torch
            ckeep = core.to(torch.uint8).contiguous()
            cr, cmem = C.c_void_p(ckeep.data_ptr()), (FI_DEVICE if ckeep.is_cuda else FI_HOST)
        else:
            ckeep = np.ascontiguousarray(core, np.uint8)
            cr, cmem = C.c_void_p(ckeep.ctypes.data), FI_HOST
        if tuple(ckeep.shape) != (n,):
            raise ValueError("core is (%d,), one per point" % n)
    mem = _same_memory(pmem, lmem, cmem)
    if num_clusters is None:
        num_clusters = int(lkeep.max()) + 1 if n else 0
    nc = max(0, int(num_clusters))
    rows = (_capi.FiClusterRow * max(nc, 1))()
    check(_capi.lib().fi_cluster_measure(ndim, n, p if n else None, lb if n else None, cr if n else None, int(num_clusters), rows, mem))
    table = np.frombuffer(rows, np.dtype(_capi.FiClusterRow), nc)          # (columns first: a row at a time costs 2 us a cluster)
    count, cores = table["count"].tolist(), table["core"].tolist()
    lo, hi, centroid = (np.ascontiguousarray(table[key][:, :ndim]) for key in ("lo", "hi", "centroid"))
    return [{"count": count[c], "core": cores[c], "lo": lo[c], "hi": hi[c], "centroid": centroid[c]} for c in range(nc)]


def keep_clusters(rows, largest=None, min_points=0):
    """A boolean mask over the rows of cluster_measure: the clusters with at least min_points members; with largest = k only
    the k of them with the most members (ties go to the lower cluster number).  Evaluated on the host, like keep_parts."""
    count = np.array([r["count"] for r in rows], np.int64)
    mask = count >= int(min_points)
    if largest is not None:
        if int(largest) < 0:
            raise ValueError("largest must be >= 0")
        order = np.argsort(-count, kind="stable")            # descending count, ties by ascending cluster number
        order = order[mask[order]][:int(largest)]
        mask = np.zeros(len(count), bool)
        mask[order] = True
    return mask


def mesh_to_sdf(mesh, sizes, max_distance=math.inf):
    """The signed distance (flat, x fastest, float32) of every point of a lattice of `sizes` to a mesh -- an IsoMesh or
    anything with `vertices` and `indices`, from a field or not: SurfaceIndex.signed_distance_field.  The sign is the parity
    of the crossings along +x, so the mesh should be closed."""
    return SurfaceIndex.from_mesh(mesh).signed_distance_field(sizes, max_distance)


class LatticeField(_PointQueries):
    """field_interpolation.hpp:97-114 `LatticeField{sizes}`: sizes[0] (x) is the fastest axis.

    dtype: "f32" (vectors fp32, reductions fp64) or "f64".  rank/nranks select a slab of the slowest
    axis (one process per GPU)."""

    def __init__(self, sizes, dtype="f32", rank=0, nranks=1, _borrowed=None):
        self.sizes = [int(s) for s in sizes]
        self.dtype = dtype
        self.rank, self.nranks = rank, nranks
        self.strides = []
        s = 1
        for n in self.sizes:
            self.strides.append(s)
            s *= n
        self._h = C.c_void_p()
        self._borrowed = _borrowed is not None
        sz = (C.c_int * len(self.sizes))(*self.sizes)
        code = {"f32": FI_F32, "f64": FI_F64}[dtype]
        if _borrowed is not None:       # a member of a LatticeGroup: the group owns the context
            self._h = C.c_void_p(_borrowed)
        elif nranks == 1:
            check(_capi.lib().fi_ctx_create(C.byref(self._h), len(self.sizes), sz, code))
        else:
            check(_capi.lib().fi_ctx_create_slab(C.byref(self._h), len(self.sizes), sz, code, rank, nranks))
        self._weights = Weights()
        self._dirty = True
        lo, hi = C.c_int(0), C.c_int(0)
        check(_capi.lib().fi_slab_range(self._h, C.byref(lo), C.byref(hi)))
        self.slab = (lo.value, hi.value)

    def point_range(self):
        """[lo, hi) of the slowest coordinate of the data points this rank has to be given (fi_slab_point_range:
        covers the cells touching the slab on every level set so far -- call after set_levels)."""
        lo, hi = C.c_float(0), C.c_float(0)
        check(_capi.lib().fi_slab_point_range(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _capi._LIB is not None and not getattr(self, "_borrowed", False):
            _capi._LIB.fi_ctx_destroy(h)
        self._h = None

    def num_dim(self):
        return len(self.sizes)

    @property
    def num_unknowns(self):
        return int(np.prod(self.sizes))

    @property
    def num_owned(self):
        n = 1
        for s in self.sizes[:-1]:
            n *= s
        return n * (self.slab[1] - self.slab[0])

    # ---- model -----------------------------------------------------------------------------
    def add_field_constraints(self, weights):
        """add_field_constraints (field_interpolation.cpp:326-341), matrix-free."""
        self._weights = weights
        w = weights._c()
        check(_capi.lib().fi_set_model(self._h, C.byref(w)))
        self._dirty = True

    # ---- data ------------------------------------------------------------------------------
    def _inside_ext(self, pos):
        fl = [math.floor(float(np.float32(p))) for p in pos]
        return all(-1 <= f <= n - 1 for f, n in zip(fl, self.sizes))

    def _cell_valid(self, pos):
        fl = [math.floor(float(np.float32(p))) for p in pos]
        return all(0 <= f and f + 1 < n for f, n in zip(fl, self.sizes))

    def _lerp_valid(self, pos):
        # kLinearInterpolation keeps a sample of multilerp(pos - 0.5, 1) when 0 <= q and q + 1 < size for q in {fl, fl + 1}
        fl = [math.floor(float(np.float32(p) - np.float32(0.5))) for p in pos]
        return all(n >= 2 and -1 <= f and f + 1 < n for f, n in zip(fl, self.sizes))

    def add_value_constraint(self, pos, value, weight):
        """add_value_constraint (field_interpolation.cpp:57-80).  False if the position was ignored."""
        pos = np.atleast_1d(np.asarray(pos, np.float32))
        if weight == 0 or not self._inside_ext(pos):
            return False
        self.add_points(weight, ValueKernel.kLinearInterpolation, 0.0, GradientKernel.kCellEdges, pos, None, None,
                        values=np.asarray([value], np.float32))
        return True

    def add_value_constraint_nearest_neighbor(self, pos, gradient, value, weight):
        """add_value_constraint_nearest_neighbor (field_interpolation.cpp:82-107)."""
        pos = np.atleast_1d(np.asarray(pos, np.float32))
        for p, n in zip(pos, self.sizes):
            q = math.floor(abs(float(p)) + 0.5) * (1 if p >= 0 else -1)     # std::round
            if q < 0 or n <= q:
                return False
        self.add_points(weight, ValueKernel.kNearestNeighbor, 0.0, GradientKernel.kCellEdges, pos,
                        np.atleast_1d(np.asarray(gradient, np.float32)), None, values=np.asarray([value], np.float32))
        return True

    def add_gradient_constraint(self, pos, gradient, weight, kernel):
        """add_gradient_constraint (field_interpolation.cpp:123-240)."""
        if int(kernel) not in (0, 1, 2):
            raise ValueError("Unknown gradient kernel: %d" % int(kernel))    # ABORT_F, cpp:238
        pos = np.atleast_1d(np.asarray(pos, np.float32))
        if weight == 0:
            return False
        if not (self._lerp_valid(pos) if int(kernel) == GradientKernel.kLinearInterpolation else self._cell_valid(pos)):
            return False                                                     # no sample kept (cpp:219) / cell_index < 0
        self.add_points(0.0, ValueKernel.kLinearInterpolation, weight, kernel, pos,
                        np.atleast_1d(np.asarray(gradient, np.float32)), None)
        return True

    def add_border_prior(self, weight):
        """The border prior of the reference's SDF application (src/sdf_field.cpp:218-246): every border lattice point
        gets the row [1] * weight = (distance to the nearest data point added so far) * weight.  After add_points."""
        check(_capi.lib().fi_add_border_prior(self._h, float(weight)))
        self._dirty = True

    def add_points(self, value_weight, value_kernel, gradient_weight, gradient_kernel, positions, normals=None,
                   point_weights=None, values=None):
        """add_points (field_interpolation.cpp:343-371); `values` (optional) generalises the fixed 0 target."""
        pp, km, _k1 = _buf(positions)
        np_, kn, _k2 = _buf(normals)
        pw, kw, _k3 = _buf(point_weights)
        pv, kv, _k4 = _buf(values)
        mem = _same_memory(km, kn, kw, kv)
        count = (_k1.numel() if hasattr(_k1, "numel") else _k1.size) // len(self.sizes)
        check(_capi.lib().fi_add_points(self._h, count, pp, np_, pw, pv, float(value_weight), int(value_kernel),
                                        float(gradient_weight), int(gradient_kernel), mem))
        self._dirty = True

    def add_volume(self, volume, value_weight, value_kernel=ValueKernel.kNearestNeighbor, min_weight=0.0):
        """The band of a DepthVolume over this lattice as data points (include/fi_hip.h fi_add_volume): its voxels with
        weight >= min_weight and |tsdf| < 1, each a value constraint tsdf * truncation with point weight W / max_weight,
        formed on the device and added as add_points adds device arrays.  No gradient rows."""
        check(_capi.lib().fi_add_volume(self._h, volume._h, float(value_weight), int(value_kernel), float(min_weight)))
        self._dirty = True

    def add_rows_coo(self, rows, cols, values, rhs):
        """Arbitrary rows of a `LinearEquation` (sparse_linear.hpp:18-22): triplets (row, col, value) with rows
        numbered from 0 within this call, and one rhs per row.  Duplicate (row, col) entries are summed in input order in
        the context's precision.  numpy arrays, or torch tensors that all live on the GPU (FI_DEVICE: no host copy)."""
        if hasattr(values, "data_ptr") and values.is_cuda:
            import torch
            if not all(hasattr(t, "data_ptr") and t.is_cuda for t in (rows, cols, rhs)):
                raise ValueError("all buffers of one call must live in the same memory (all host or all device)")
            trip = torch.empty((values.numel(), 3), dtype=torch.int32, device=values.device)    # fi_triplet: 12 bytes
            trip[:, 0], trip[:, 1] = rows, cols
            trip[:, 2] = values.to(torch.float32).contiguous().view(torch.int32)
            b = rhs.to(torch.float32).contiguous()
            torch.cuda.synchronize(values.device)                # the library works on a stream of its own
            check(_capi.lib().fi_add_rows_coo(self._h, b.numel(), trip.shape[0], C.c_void_p(trip.data_ptr()),
                                              C.c_void_p(b.data_ptr()), FI_DEVICE))
            self._dirty = True
            return
        trip = np.empty(len(values), dtype=[("row", np.int32), ("col", np.int32), ("value", np.float32)])
        trip["row"], trip["col"], trip["value"] = rows, cols, values
        b = np.ascontiguousarray(rhs, np.float32)
        check(_capi.lib().fi_add_rows_coo(self._h, b.size, trip.size, C.c_void_p(trip.ctypes.data),
                                          C.c_void_p(b.ctypes.data), FI_HOST))
        self._dirty = True

    def clear_points(self):
        check(_capi.lib().fi_clear_points(self._h))
        self._dirty = True

    # ---- distributed -----------------------------------------------------------------------
    def comm_init(self, unique_id):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        check(_capi.lib().fi_comm_init(self._h, buf))

    def comm_info(self):
        """fi_comm_info: what the slab transport looks like from inside -- the ranks RCCL itself counts (ncclCommCount), this
        rank's index and device there, the kind of transport, ghost planes per exchange and their bytes."""
        out = (C.c_long * 7)()
        check(_capi.lib().fi_comm_info(self._h, out))
        kind = {0: "none", 1: "rccl", 2: "host-staged test transport"}.get(out[3], "?")
        return {"ranks": out[0], "rank": out[1], "device": out[2], "transport": kind, "halo_planes": out[4],
                "halo_planes_stored": out[5], "plane_bytes": out[6], "halo_bytes_per_exchange": out[4] * out[6]}

    def comm_init_host(self, name, create):
        """fi_comm_init_host: the host-staged TEST transport for ranks that share one GPU."""
        check(_capi.lib().fi_comm_init_host(self._h, name.encode(), 1 if create else 0))

    # ---- assemble / solve --------------------------------------------------------------------
    def assemble(self):
        """as_sparse_matrix_float + make_square + A^T b (sparse_linear.cpp:59-70,105-113,120) on the GPU."""
        check(_capi.lib().fi_assemble(self._h))
        self._dirty = False

    def _ready(self):
        if self._dirty:
            self.assemble()

    def _out(self, like):
        if like is not None and hasattr(like, "data_ptr") and like.is_cuda:
            import torch
            return torch.empty(self.num_owned, dtype=torch.float32, device=like.device)
        return np.empty(self.num_owned, np.float32)

    def solve_cg(self, guess=None, max_iterations=0, error_tolerance=0.0, out=None):
        """-> (x, iterations, relative residual) or None on solver breakdown."""
        self._ready()
        g, kg, _kg = _buf(guess)
        if out is None:
            out = self._out(guess)
        o, ko, _ko = _buf(out)
        mem = _same_memory(kg, ko)
        it, rel = C.c_int(0), C.c_float(0)
        try:
            check(_capi.lib().fi_solve_cg(self._h, g, int(max_iterations), float(error_tolerance), o, C.byref(it),
                                          C.byref(rel), mem))
        except FiError as e:
            if e.code == 6:     # FI_ERR_BREAKDOWN: the reference logs a warning and returns {}
                return None
            raise
        return out, it.value, rel.value

    # ---- robust fits (include/fi_hip.h, "robust fits") -------------------------------------------------
    def point_count(self):
        """The number of data points: every add_points batch in call order, the border prior's rows left out."""
        n = C.c_long(0)
        check(_capi.lib().fi_point_count(self._h, C.byref(n)))
        return n.value

    def _per_point(self, like):
        n = self.point_count()
        if like is not None and hasattr(like, "data_ptr") and like.is_cuda:
            import torch
            t = torch.empty(n, dtype=torch.float32, device=like.device)
            return t, C.c_void_p(t.data_ptr())
        a = np.empty(n, np.float32)
        return a, C.c_void_p(a.ctypes.data)

    def point_residuals(self, solution=None):
        """Every data point's residual against `solution` (this context's owned values, host or device) or, with None, the
        last solve's solution where it lives: the root of the summed squares of the point's rows at unit point weight; -1
        for a point that emits no row.  Results live where `solution` lives (numpy for None)."""
        s, smem, _keep = _buf(solution)
        r, rp = self._per_point(solution)
        check(_capi.lib().fi_point_residuals(self._h, s, rp, FI_HOST if smem is None else smem))
        return r

    def robust_reweight(self, solution=None, loss="huber", tuning=0.0, scale=0.0):
        """One step of iteratively reweighted least squares: residuals -> scale (1.4826 x their median unless given) ->
        weight factors omega -> point weights base * sqrt(omega); the rows are emitted again and the next solve assembles
        them.  loss: "huber", "cauchy" or "tukey"; tuning 0: the loss's default constant.  -> (omega, scale); scale 0 means
        more than half of the points fit exactly and nothing was changed."""
        s, smem, _keep = _buf(solution)
        om, op = self._per_point(solution)
        opt = _capi.FiRobustOptions(_capi.FI_LOSS[loss], float(tuning), float(scale), 0, 0.0)
        sc = C.c_float(0)
        check(_capi.lib().fi_robust_reweight(self._h, s, C.byref(opt), op, C.byref(sc), FI_HOST if smem is None else smem))
        if sc.value != 0.0:
            self._dirty = True
        return om, sc.value

    def reset_point_weights(self):
        """Back to the caller's point weights (every omega 1); the next solve assembles again."""
        check(_capi.lib().fi_reset_point_weights(self._h))
        self._dirty = True

    def solve_robust(self, guess=None, loss="huber", tuning=0.0, scale=0.0, rounds=5, weight_tolerance=0.0, max_iterations=0,
                     error_tolerance=0.0):
        """A plain solve, then up to `rounds` reweighted ones, each from the previous field, under the solver options this
        context carries.  Ends early at scale 0 or when no omega moved by weight_tolerance.  Afterwards the context holds the
        last weights.  -> (field, omega, stats dict: rounds, iterations of all solves, scale, max_weight_change, points_used,
        points_zeroed, reweight_ms)"""
        self._ready()
        g, kg, _kg = _buf(guess)
        out = self._out(guess)
        o, ko, _ko = _buf(out)
        om, op = self._per_point(guess)
        opt = _capi.FiRobustOptions(_capi.FI_LOSS[loss], float(tuning), float(scale), int(rounds), float(weight_tolerance))
        st = _capi.FiRobustStats()
        check(_capi.lib().fi_solve_robust(self._h, g, C.byref(opt), int(max_iterations), float(error_tolerance), o, op,
                                          C.byref(st), _same_memory(kg, ko)))
        return out, om, {f: getattr(st, f) for f, _ in st._fields_}

    def iso_surface(self, solution=None, iso=0.0, normals=True, largest=None, min_size=None, parts=False, simplify=None,
                    smooth=None):
        """The iso-contour (2-D) / iso-surface (3-D) f = iso of `solution` (this context's owned values, host or device) or,
        with None, of the last solve's solution where it lives on the device -- the step src/sdf_field.cpp:605-613 takes
        after the solve.  A slab context returns its piece (merge_meshes joins them).  -> IsoMesh
        largest = k / min_size = s: only the k largest connected parts / the parts of at least that area (2-D: length) are
        kept (keep_parts), chosen and cut out on the device before the one copy to the host; parts=True: -> (IsoMesh,
        MeshParts of that mesh).  simplify = cell or (cell, placement): the mesh (after the selection, if any) is made
        coarser on the device by simplify_mesh's vertex clustering before the copy; parts=True then describes that mesh.
        smooth = iterations or a dict of smooth_mesh's keywords: the mesh is faired on the device by smooth_mesh after the
        selection and before the simplification (whose quadrics then fit the faired surface)."""
        h = C.c_void_p()
        if solution is None:
            check(_capi.lib().fi_iso_extract(self._h, None, float(iso), FI_HOST, C.byref(h)))
        else:
            s, mem, _keep = _buf(solution)
            check(_capi.lib().fi_iso_extract(self._h, s, float(iso), mem, C.byref(h)))
        return _finish_mesh(h, len(self.sizes), normals, largest, min_size, parts, simplify, smooth)

    def dual_contour(self, solution=None, iso=0.0, gradients=None, normals=True, largest=None, min_size=None, parts=False,
                     simplify=None, smooth=None):
        """The dual contour (2-D: segments, 3-D: triangles) of `solution` (this context's owned values, host or device) or,
        with None, of the last solve's solution where it lives on the device: one vertex per crossed cell, fitted to the
        corner gradients so that sharp corners survive (include/fi_hip.h fi_dual_contour).  gradients: (num_owned, ndim)
        in the same memory as `solution`, or None for central differences of f - iso.  Undivided contexts only.  -> IsoMesh
        (keys: the lattice index of each vertex's cell).  largest, min_size, parts, simplify, smooth: as iso_surface's."""
        s, smem, _ks = _buf(solution)
        g, gmem, _kg = _buf(gradients)
        mem = _same_memory(smem, gmem)
        h = C.c_void_p()
        check(_capi.lib().fi_dual_contour(self._h, s, g, float(iso), mem, C.byref(h)))
        return _finish_mesh(h, len(self.sizes), normals, largest, min_size, parts, simplify, smooth)

    def sample(self, positions, solution=None, gradients=False, cubic=False, fill=float("nan")):
        """Values (n,) -- and with gradients=True also gradients (n, ndim) -- of `solution` (this context's owned values) or,
        with None, of the last solve's solution where it lives on the device, at `positions` (n x ndim, global lattice
        coordinates, x fastest).  Multilinear, or Catmull-Rom with cubic=True; points outside the lattice get `fill`.  A slab
        context's call is collective and every rank receives every point (include/fi_hip.h fi_sample)."""
        s, smem, _keep = _buf(solution)

        def call(n, p, mode, fl, v, g, mem):
            return _capi.lib().fi_sample(self._h, s, n, p, mode, fl, v, g, mem)
        return _sample(call, len(self.sizes), positions, [smem], gradients, cubic, fill)

    def raycast(self, origins, directions, solution=None, iso=0.0, step=1.0, refine=4, side="front", t_min=0.0, t_max=math.inf,
                positions=False, normals=False):
        """raycast_field against `solution` (this context's owned values, in the rays' memory) or, with None, against the
        last solve's solution where it lives on the device (an fp64 one rounded to fp32 once, as iso_surface does): the field
        itself is marched, no mesh is built.  2-D or 3-D, undivided contexts only (include/fi_hip.h fi_raycast_field)."""
        opt = _march_options(iso, step, refine, side, 0.0)
        s, smem, _keep = _buf(solution)

        def call(n, o, d, tp, pp, np_, sp, mem):
            return _capi.lib().fi_raycast_field(self._h, s, C.byref(opt), n, o, d, float(t_min), float(t_max), tp, pp, np_, sp, mem)
        return _march_rays(call, len(self.sizes), origins, directions, positions, normals, [smem])

    def render(self, camera, solution=None, iso=0.0, step=1.0, refine=4, side="front", positions=False, normals=False,
               incidence=False, device=False):
        """render_field of `solution` (this context's owned values; a device tensor with device=True) or, with None, of the
        last solve's solution where it lives on the device.  3-D, undivided contexts only; numpy arrays out, or torch
        tensors with device=True (include/fi_hip.h fi_render_field)."""
        opt = _march_options(iso, step, refine, side, 0.0)
        s, smem, _keep = _buf(solution)
        if smem is not None and (smem == FI_DEVICE) != bool(device):
            raise ValueError("solution and the outputs live in the same memory: device=True with a device tensor")

        def call(cam, dp, pp, np_, ip, mem):
            return _capi.lib().fi_render_field(self._h, s, C.byref(opt), cam, dp, pp, np_, ip, mem)
        return _march_image(call, camera, positions, normals, incidence, device)

    def _point_op(self, op):
        return functools.partial(getattr(_capi.lib(), "fi_" + op), self._h)

    def _point_ndim(self):
        return len(self.sizes)

    _point_count = point_count

    def distance_field(self, max_distance=math.inf, indices=False, device=False):
        """LatticeField.nearest of every lattice point (x fastest), flat: numpy arrays, or torch tensors with device=True."""
        def call(d, i, mem):
            return _capi.lib().fi_distance_field(self._h, float(max_distance), d, i, mem)
        return _distance_field(call, self.num_unknowns, indices, device)

    def redistance(self, solution=None, iso=0.0, method="iso", max_distance=math.inf, primitives=False, device=False):
        """The signed distance of every lattice point (x fastest) to the iso-surface f = iso of `solution` (this context's
        owned values, host or device) or, with None, of the last solve's solution where it lives: negative inside (method
        "iso": fi_iso_extract's mesh, inside is f < iso; "dual": fi_dual_contour's, inside is f - iso <= 0), +-inf beyond
        max_distance (include/fi_hip.h fi_redistance).  Undivided contexts only.  -> distances (numpy, or torch tensors with
        device=True), or with primitives=True (distances, primitive indices, the IsoMesh they index)"""
        s, smem, _keep = _buf(solution)
        _same_memory(smem, FI_DEVICE if device else FI_HOST)
        m = _surface_method(method)

        def call(d, i, h, mem):
            return _capi.lib().fi_redistance(self._h, s, float(iso), m, float(max_distance), d, i, h, mem)
        return _redistance(call, self.num_unknowns, primitives, device, len(self.sizes))

    def register(self, points, iso=0.0, method="iso", mode="plane", max_iterations=30, max_distance=math.inf,
                 rotation_tolerance=1e-6, translation_tolerance=1e-6, loss=None, scale=0.0, tuning=0.0, initial=None,
                 transformed=False, distances=False):
        """register_points of `points` (n, ndim) to the surface f = iso of the last solve's solution: the mesh of
        iso_surface (method "iso") or of dual_contour with central differences ("dual") is extracted, searched and
        registered to on the device and never copied to the host.  Undivided contexts only.  -> register_points' dict"""
        opt = _register_options(mode, max_iterations, max_distance, rotation_tolerance, translation_tolerance, loss, scale, tuning)
        h = C.c_void_p()
        if _surface_method(method) == 0:
            check(_capi.lib().fi_iso_extract(self._h, None, float(iso), FI_HOST, C.byref(h)))
        else:
            check(_capi.lib().fi_dual_contour(self._h, None, None, float(iso), FI_HOST, C.byref(h)))
        try:
            return _register_to_mesh(h, None, len(self.sizes), points, opt, initial, transformed, distances)
        finally:
            _capi.lib().fi_mesh_destroy(h)

    def set_verify_residual(self, on):
        """FI_OPT_VERIFY_RESIDUAL: True (default) checks b - A x at convergence and restarts CG if fp32 drift
        left it above the tolerance; False stops on the recurrence residual alone, like the reference."""
        check(_capi.lib().fi_set_option(self._h, 1, 1.0 if on else 0.0))

    def set_levels(self, levels, coarse_tolerance=None):
        """FI_OPT_LEVELS: build `levels` coarser replicas at the next assemble; solve_cg(guess=None) then starts
        from a coarse-to-fine cascade (src/sdf_field.cpp:272-288 generalised, on the device)."""
        check(_capi.lib().fi_set_option(self._h, 2, float(levels)))
        if coarse_tolerance is not None:
            check(_capi.lib().fi_set_option(self._h, 3, float(coarse_tolerance)))
        self._dirty = True

    def set_multigrid(self, on=True):
        """FI_OPT_MULTIGRID: V-cycle preconditioned CG over the levels of set_levels()."""
        check(_capi.lib().fi_set_option(self._h, 4, 1.0 if on else 0.0))
        self._dirty = True

    def set_mixed_precision(self, on=True):
        """FI_OPT_MIXED_PRECISION (dtype="f64" fields with levels + multigrid): CG in fp64, V-cycle in fp32."""
        check(_capi.lib().fi_set_option(self._h, 5, 1.0 if on else 0.0))
        self._dirty = True

    def set_field_tolerance(self, tol):
        """FI_OPT_FIELD_TOLERANCE (V-cycle PCG; undivided lattices and up to 16 slabs): stop when the field is within `tol` (relative, maximum
        norm) of the converged solution by the solver's own measure -- the last step times sigma / (1 - sigma), sigma the
        slowest mean decay of the residual norm over the recent windows and the whole solve, doubled (include/fi_hip.h) --
        instead of at a residual; the `tol` of solve_cg is then ignored.  0: the residual rule.  stats(): field_estimate, field_per_residual,
        stop_residual, field_rounds (1 only when the field test ended the solve).  Where the rule cannot run -- multigrid off,
        no coarser level built (a small lattice, add_rows_coo rows), more than 16 slabs, a finest level of replicated copies --
        the solve stops by the residual at solve_cg's `tol` and stats() says so: field_estimate -1, field_rounds 0."""
        check(_capi.lib().fi_set_option(self._h, 12, float(tol)))

    def set_cheb_smoother(self, degree=0, ratio=0.0):
        """FI_OPT_MG_CHEB_DEGREE / FI_OPT_MG_CHEB_RATIO: the full-operator Chebyshev smoother's degree and interval; 0: by the dimension."""
        check(_capi.lib().fi_set_option(self._h, 14, float(degree)))
        check(_capi.lib().fi_set_option(self._h, 15, float(ratio)))
        self._dirty = True

    def set_kcycle(self, levels):
        """FI_OPT_MG_KCYCLE: the first `levels` coarse levels corrected by two flexible-CG steps each (a K-cycle); 0: the V-cycle."""
        check(_capi.lib().fi_set_option(self._h, 13, float(levels)))
        self._dirty = True

    def set_polynomial(self, terms, ratio=None):
        """FI_OPT_POLY_TERMS / FI_OPT_POLY_RATIO: CG preconditioned by a Chebyshev polynomial of `terms` terms
        (0: the Jacobi diagonal).  No re-assembly needed."""
        check(_capi.lib().fi_set_option(self._h, 6, float(terms)))
        if ratio is not None:
            check(_capi.lib().fi_set_option(self._h, 7, float(ratio)))

    def set_mg_smoother(self, polynomial=True, safe_factor=None, terms=None, ratio=None):
        """FI_OPT_MG_SMOOTHER / FI_OPT_MG_SAFE_FACTOR / FI_OPT_MG_TERMS / FI_OPT_MG_RATIO: the V-cycle's smoother on fp32 3-D
        levels -- the polynomial in A_model + f diag(A_data) (default; `terms` terms over [hi / ratio, hi]) or the Chebyshev
        polynomial in the full operator."""
        check(_capi.lib().fi_set_option(self._h, 8, 1.0 if polynomial else 0.0))
        if safe_factor is not None:
            check(_capi.lib().fi_set_option(self._h, 9, float(safe_factor)))
        if terms is not None:
            check(_capi.lib().fi_set_option(self._h, 10, float(terms)))
        if ratio is not None:
            check(_capi.lib().fi_set_option(self._h, 11, float(ratio)))
        self._dirty = True

    def jacobi(self, guess, num_iterations, weight):
        self._ready()
        g, kg, _kg = _buf(guess)
        out = self._out(guess)
        o, ko, _ko = _buf(out)
        check(_capi.lib().fi_jacobi(self._h, g, int(num_iterations), float(weight), o, _same_memory(kg, ko)))
        return out

    def error_map(self, solution):
        """generate_error_map (field_interpolation.cpp:402-429) on the device: fi_error_map."""
        self._ready()
        g, kg, _kg = _buf(solution)
        out = self._out(solution)
        o, ko, _ko = _buf(out)
        check(_capi.lib().fi_error_map(self._h, g, o, _same_memory(kg, ko)))
        return out

    def tile_pass(self, guess, tile_size=16):
        """tile_solver_square (sparse_linear.cpp:246-390) on the device: fi_tile_pass."""
        self._ready()
        g, kg, _kg = _buf(guess)
        out = self._out(guess)
        o, ko, _ko = _buf(out)
        check(_capi.lib().fi_tile_pass(self._h, g, int(tile_size), o, _same_memory(kg, ko)))
        return out

    def solution_f64(self):
        out = np.empty(self.num_owned, np.float64)
        check(_capi.lib().fi_get_solution_f64(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def true_residual(self):
        r = C.c_double(0)
        check(_capi.lib().fi_true_residual(self._h, C.byref(r)))
        return r.value

    # ---- test / measurement hooks --------------------------------------------------------------
    def apply_AtA(self, x):
        self._ready()
        xx = np.ascontiguousarray(x, np.float64)
        y = np.empty(self.num_owned, np.float64)
        dp = C.POINTER(C.c_double)
        check(_capi.lib().fi_apply_AtA_f64(self._h, xx.ctypes.data_as(dp), y.ctypes.data_as(dp)))
        return y

    def Atb(self):
        self._ready()
        out = np.empty(self.num_owned, np.float64)
        check(_capi.lib().fi_get_Atb_f64(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def diag(self):
        self._ready()
        out = np.empty(self.num_owned, np.float64)
        check(_capi.lib().fi_get_diag_f64(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def stats(self):
        s = FiStats()
        check(_capi.lib().fi_get_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in FiStats._fields_}

    def time_apply(self, reps=20):
        self._ready()
        ms = C.c_double(0)
        check(_capi.lib().fi_time_apply(self._h, reps, C.byref(ms)))
        return ms.value


class LatticeGroup:
    """All slabs of a decomposition in one process on one GPU (loop-back test facility, fi_hip.h
    "loop-back group"): same kernels and slab rules as the one-process-per-GPU RCCL path."""

    def __init__(self, sizes, nranks, dtype="f32"):
        self.sizes = [int(s) for s in sizes]
        self.dtype = dtype
        self._g = C.c_void_p()
        sz = (C.c_int * len(self.sizes))(*self.sizes)
        check(_capi.lib().fi_group_create(C.byref(self._g), len(self.sizes), sz, {"f32": FI_F32, "f64": FI_F64}[dtype],
                                          nranks))
        self.members = [LatticeField(self.sizes, dtype=dtype, rank=r, nranks=nranks,
                                     _borrowed=_capi.lib().fi_group_rank(self._g, r)) for r in range(nranks)]

    def __del__(self):
        g = getattr(self, "_g", None)
        if g and _capi._LIB is not None:
            for m in getattr(self, "members", []):
                m._h = None
            _capi._LIB.fi_group_destroy(g)
            self._g = None

    @property
    def num_unknowns(self):
        return int(np.prod(self.sizes))

    def add_field_constraints(self, weights):
        for m in self.members:
            m.add_field_constraints(weights)

    def add_points(self, *a, **kw):
        for m in self.members:          # every rank sees every point and keeps the cells touching its slab
            m.add_points(*a, **kw)

    def set_levels(self, levels, coarse_tolerance=None):
        for m in self.members:
            m.set_levels(levels, coarse_tolerance)

    def set_multigrid(self, on=True):
        for m in self.members:
            m.set_multigrid(on)

    def set_mixed_precision(self, on=True):
        for m in self.members:
            m.set_mixed_precision(on)

    def set_field_tolerance(self, tol):
        for m in self.members:
            m.set_field_tolerance(tol)

    def set_polynomial(self, terms, ratio=None):
        for m in self.members:
            m.set_polynomial(terms, ratio)

    def set_mg_smoother(self, polynomial=True, safe_factor=None, terms=None, ratio=None):
        for m in self.members:
            m.set_mg_smoother(polynomial, safe_factor, terms, ratio)

    def set_cheb_smoother(self, degree=0, ratio=0.0):
        for m in self.members:
            m.set_cheb_smoother(degree, ratio)

    def set_kcycle(self, levels):
        for m in self.members:
            m.set_kcycle(levels)

    def assemble(self):
        check(_capi.lib().fi_group_assemble(self._g))
        for m in self.members:
            m._dirty = False

    def apply_AtA(self, x):
        xx = np.ascontiguousarray(x, np.float64)
        y = np.empty(self.num_unknowns, np.float64)
        dp = C.POINTER(C.c_double)
        check(_capi.lib().fi_group_apply_AtA_f64(self._g, xx.ctypes.data_as(dp), y.ctypes.data_as(dp)))
        return y

    def Atb(self):
        return np.concatenate([m.Atb() for m in self.members])

    def diag(self):
        return np.concatenate([m.diag() for m in self.members])

    def solve_cg(self, guess=None, max_iterations=0, error_tolerance=0.0):
        g = None if guess is None else np.ascontiguousarray(guess, np.float32)
        out = np.empty(self.num_unknowns, np.float32)
        it, rel = C.c_int(0), C.c_float(0)
        check(_capi.lib().fi_group_solve_cg(self._g, None if g is None else C.c_void_p(g.ctypes.data), int(max_iterations),
                                            float(error_tolerance), C.c_void_p(out.ctypes.data), C.byref(it), C.byref(rel)))
        return out, it.value, rel.value

    def stats(self):
        return self.members[0].stats()

    def tile_pass(self, guess, tile_size=16):
        g = np.ascontiguousarray(guess, np.float32)
        out = np.empty(self.num_unknowns, np.float32)
        fp = C.POINTER(C.c_float)
        check(_capi.lib().fi_group_tile_pass(self._g, g.ctypes.data_as(fp), int(tile_size), out.ctypes.data_as(fp)))
        return out

    def error_map(self, solution):
        s = np.ascontiguousarray(solution, np.float32)
        out = np.empty(self.num_unknowns, np.float32)
        fp = C.POINTER(C.c_float)
        check(_capi.lib().fi_group_error_map(self._g, s.ctypes.data_as(fp), out.ctypes.data_as(fp)))
        return out

    def solution_f64(self):
        out = np.empty(self.num_unknowns, np.float64)
        check(_capi.lib().fi_group_get_solution_f64(self._g, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def true_residual(self):
        r = C.c_double(0)
        check(_capi.lib().fi_group_true_residual(self._g, C.byref(r)))
        return r.value

    def iso_surface(self, field=None, iso=0.0, normals=True):
        """The pieces (one IsoMesh per slab, rank order) of the iso-contour of `field` (the WHOLE lattice, host) or, with
        None, of the members' last solution.  merge_meshes(pieces) is the undivided mesh."""
        hs = (C.c_void_p * len(self.members))()
        f = None if field is None else np.ascontiguousarray(field, np.float32).reshape(-1)
        check(_capi.lib().fi_group_iso_extract(self._g, None if f is None else C.c_void_p(f.ctypes.data), float(iso), hs))
        out = []
        try:
            for r in range(len(self.members)):
                h, hs[r] = hs[r], None
                out.append(_take_mesh(C.c_void_p(h), len(self.sizes), normals))
        finally:
            for h in hs:
                if h:
                    _capi.lib().fi_mesh_destroy(C.c_void_p(h))
        return out

    def sample(self, positions, field=None, gradients=False, cubic=False, fill=float("nan")):
        """LatticeField.sample of `field` (the WHOLE lattice) or, with None, of the members' last solution; host arrays only.
        The results are those of the undivided lattice."""
        f = None if field is None else np.ascontiguousarray(field, np.float32).reshape(-1)
        pos = np.ascontiguousarray(positions, np.float32)

        def call(n, p, mode, fl, v, g, mem):
            return _capi.lib().fi_group_sample(self._g, None if f is None else C.c_void_p(f.ctypes.data), n, p, mode, fl, v, g)
        return _sample(call, len(self.sizes), pos, [], gradients, cubic, fill)


# ---- free functions with the reference's names ---------------------------------------------------

def sdf_from_points(sizes, weights, positions, normals=None, point_weights=None, dtype="f32", rank=0, nranks=1):
    """sdf_from_points (field_interpolation.cpp:373-400): model rows, then add_points with target 0."""
    if positions is None:
        raise ValueError("positions is null")            # CHECK_NOTNULL_F, cpp:382
    field = LatticeField(sizes, dtype=dtype, rank=rank, nranks=nranks)
    field.add_field_constraints(weights)
    field.add_points(weights.data_pos, weights.value_kernel, weights.data_gradient, weights.gradient_kernel,
                     positions, normals, point_weights)
    return field


def sdf_from_unoriented_points(sizes, weights, positions, k=16, viewpoints=None, directions=None, propagate=False, **kw):
    """sdf_from_points for a cloud without normals: a PointIndex over `positions`, its estimate_normals(k, viewpoints,
    directions, propagate), then sdf_from_points(sizes, weights, positions, normals, **kw).  Without viewpoints or
    directions and without propagate=True the normals carry no consistent orientation, and neither does the field's sign;
    with propagate=True the guides are optional (PointIndex.orient_normals)."""
    if positions is None:
        raise ValueError("positions is null")
    normals = PointIndex(positions, ndim=len(sizes)).estimate_normals(k=k, viewpoints=viewpoints, directions=directions,
                                                                      device=hasattr(positions, "is_cuda") and positions.is_cuda,
                                                                      propagate=propagate)
    return sdf_from_points(sizes, weights, positions, normals, **kw)


# ---- depth images (include/fi_hip.h fi_depth_unproject, fi_volume_integrate) ------------------------------

class Camera:
    """A pinhole camera for depth images (include/fi_hip.h fi_camera): pose (3, 4) float32 = [R | t], world (lattice
    coordinates) to camera; it looks along +z, image x goes right, y down; pixel (row, col) has its centre at (col + 0.5,
    row + 0.5).  kind: "range" (distance along the pixel's ray, what SurfaceIndex.render_depth writes) or "z" (depth along
    the optical axis)."""

    def __init__(self, pose, fx, fy, cx, cy, width, height, kind="range"):
        self.pose = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(3, 4))
        self.fx, self.fy, self.cx, self.cy = (float(np.float32(v)) for v in (fx, fy, cx, cy))
        self.width, self.height = int(width), int(height)
        if kind not in _capi.FI_DEPTH:
            raise ValueError("kind must be 'range' or 'z' (got %r)" % (kind,))
        self.kind = kind

    def _c(self):
        return _capi.FiCamera((C.c_float * 12)(*self.pose.reshape(-1).tolist()), self.fx, self.fy, self.cx, self.cy, self.width,
                              self.height, _capi.FI_DEPTH[self.kind])


def camera_look_at(eye, target, up, fov_y, width, height, kind="range"):
    """The Camera whose pixel-centre rays are those of SurfaceIndex.render_depth(eye, target, up, fov_y, width, height): the
    rows of R are that function's right, -top and fwd, t = -R eye, fx = fy = height / (2 tan(fov_y / 2)), cx = width / 2,
    cy = height / 2; computed in float64 and rounded to float32 once."""
    eye = np.asarray(eye, np.float64).reshape(3)
    fwd = np.asarray(target, np.float64).reshape(3) - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.asarray(up, np.float64).reshape(3))
    right /= np.linalg.norm(right)
    top = np.cross(right, fwd)
    R = np.stack([right, -top, fwd])
    f = height / (2.0 * math.tan(0.5 * fov_y))
    return Camera(np.concatenate([R, -(R @ eye)[:, None]], axis=1), f, f, 0.5 * width, 0.5 * height, width, height, kind)


def _count(keep):
    return keep.numel() if hasattr(keep, "numel") else keep.size


def depth_to_points(camera, depth, max_jump=math.inf, positions=True, normals=True, incidence=True, valid=True, compact=False):
    """A depth image (height, width) as oriented points on the device (include/fi_hip.h fi_depth_unproject): the tuple of
    those asked for among positions (h w, 3), normals (h w, 3), incidence (h w,) float32 and valid (h w,) bool, in pixel
    order.  A pixel is valid when its depth is finite and > 0; its normal is the cross product of the image's own
    differences (central where both neighbours are valid and within max_jump in depth, else one-sided), turned towards the
    eye; incidence is the cosine between the normal and the ray back to the eye, in (0, 1].  An invalid pixel has a NaN
    position, a pixel without a normal a zero normal and a zero incidence.  compact=True drops the invalid pixels.  numpy
    in, numpy out; a torch tensor on the GPU in, tensors on that GPU out."""
    d, mem, keep = _buf(depth)
    n = camera.width * camera.height
    if _count(keep) != n:
        raise ValueError("depth: %d values for a %d x %d image" % (_count(keep), camera.height, camera.width))
    dev = keep.device if mem == FI_DEVICE else None
    pos, pp = _cloud_out(dev, (n, 3), np.float32) if positions else (None, None)
    nrm, pn = _cloud_out(dev, (n, 3), np.float32) if normals else (None, None)
    inc, pi = _cloud_out(dev, (n,), np.float32) if incidence else (None, None)
    val, pv = _cloud_out(dev, (n,), np.uint8) if (valid or compact) else (None, None)
    cam = camera._c()
    check(_capi.lib().fi_depth_unproject(C.byref(cam), d, float(max_jump), pp, pn, pi, pv, mem))
    mask = _as_mask(val) if val is not None else None
    out = [a for a in (pos, nrm, inc) if a is not None]
    if compact:
        out = [a[mask] for a in out]
        mask = mask[mask]
    return tuple(out) + ((mask,) if valid else ())


def _flat_images(images):
    """a list of images (or one array of them back to back) as one flat float32 array / tensor"""
    if images is None or not isinstance(images, (list, tuple)):
        return images
    if any(hasattr(a, "data_ptr") for a in images):
        import torch
        return torch.cat([torch.as_tensor(a).reshape(-1).float() for a in images])
    return np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in images]) if images else np.zeros(0, np.float32)


class DepthVolume:
    """A truncated signed distance volume over a 3-D lattice on the device (include/fi_hip.h fi_volume_integrate): for every
    lattice point tsdf (fp32, 1 at first: free space, in units of `truncation`) and weight (fp32, 0 at first: never seen).
    integrate() fuses depth images into it; constraints() / LatticeField.add_volume hand its band to the solve.

    channels = 1 .. 4 adds colour (include/fi_hip.h fi_volume_integrate_colour): that many fp32 channels and one colour weight
    per lattice point, 0 at first, which integrate(colours=...) averages over the views.  Two chains lead on from there:
    vol.sample_colours(mesh.vertices) colours a mesh of iso_surface or dual_contour, and, with positions, colours, weights =
    vol.colour_constraints(), field.add_points(w, ValueKernel.kLinearInterpolation, 0.0, GradientKernel.kNearestNeighbor,
    positions, values=colours[:, k], point_weights=weights) completes channel k over the lattice by a solve."""

    def __init__(self, sizes, truncation, max_weight=64.0, channels=0):
        self.sizes = [int(s) for s in sizes]
        self.truncation, self.max_weight = float(truncation), float(max_weight)
        self.channels = int(channels)
        self._h = C.c_void_p()
        sz = (C.c_int * len(self.sizes))(*self.sizes)
        check(_capi.lib().fi_volume_create(C.byref(self._h), len(self.sizes), sz, self.truncation, self.max_weight))
        if self.channels:
            check(_capi.lib().fi_volume_set_channels(self._h, self.channels))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _capi._LIB is not None:
            _capi._LIB.fi_volume_destroy(h)
        self._h = None

    @property
    def num_voxels(self):
        return int(np.prod(self.sizes))

    def integrate(self, cameras, depths, incidences=None, image_weights=None, min_incidence=0.5, colours=None, colour_band=1.0):
        """Fuses the depth images `depths` (a list of (height, width) arrays, or one array with the images back to back) seen
        by `cameras` into the volume, in that order.  incidences (optional, same layout; depth_to_points gives them) scale
        each sample's distance along the ray into one along the normal and weigh it; samples below min_incidence are left
        out.  image_weights (optional): one factor per image.  colours (optional, a volume with channels): a list of (height,
        width, channels) images, or one flat array of them back to back, of any dtype, converted to float32 without scaling;
        a voxel within colour_band * truncation of the surface averages its pixel's colour under the weight of the depth
        sample, and tsdf and weight come out as without colours.  numpy arrays, or torch tensors on the GPU."""
        cameras = [cameras] if isinstance(cameras, Camera) else list(cameras)
        m = len(cameras)
        total = sum(c.width * c.height for c in cameras)
        d, dm, dk = _buf(_flat_images(depths))
        q, qm, qk = _buf(_flat_images(incidences))
        w, wm, wk = _buf(image_weights)
        c, cm, ck = _buf(_flat_images(colours))
        for name, keep, want in (("depths", dk, total), ("incidences", qk, total), ("image_weights", wk, m),
                                 ("colours", ck, total * self.channels)):
            if (keep is not None or name == "depths") and (0 if keep is None else _count(keep)) != want:
                raise ValueError("%s: %d values, %d expected" % (name, 0 if keep is None else _count(keep), want))
        if dm == FI_DEVICE and wk is not None and wm != FI_DEVICE:       # a short host list beside device images
            import torch
            wk = torch.as_tensor(wk).to(dk.device)
            w, wm = C.c_void_p(wk.data_ptr()), FI_DEVICE
        mem = _same_memory(dm, qm, wm, cm)
        cams = (_capi.FiCamera * max(m, 1))(*[cam._c() for cam in cameras])
        if colours is None:
            check(_capi.lib().fi_volume_integrate(self._h, m, cams, d if total else None, q if total else None, w if m else None,
                                                  float(min_incidence), mem))
        else:
            check(_capi.lib().fi_volume_integrate_colour(self._h, m, cams, d if total else None, q if total else None,
                                                         w if m else None, float(min_incidence), c if total else None,
                                                         float(colour_band), mem))
        return self

    def _read(self, which, device):
        a, p = _cloud_out("cuda" if device else None, (self.num_voxels,), np.float32)
        check(_capi.lib().fi_volume_copy(self._h, p if which == 0 else None, p if which == 1 else None,
                                         FI_DEVICE if device else FI_HOST))
        return a

    def tsdf(self, device=False):
        """the truncated signed distances in units of `truncation`, (num_voxels,) float32, x fastest"""
        return self._read(0, device)

    def weight(self, device=False):
        """the weights, (num_voxels,) float32, x fastest"""
        return self._read(1, device)

    def load(self, tsdf, weight):
        """sets both arrays (num_voxels values each): resumes a fusion"""
        t, tm, tk = _buf(tsdf)
        w, wm, wk = _buf(weight)
        if _count(tk) != self.num_voxels or _count(wk) != self.num_voxels:
            raise ValueError("tsdf and weight must hold %d values each" % self.num_voxels)
        check(_capi.lib().fi_volume_load(self._h, t, w, _same_memory(tm, wm)))
        return self

    # ---- colour (include/fi_hip.h fi_volume_integrate_colour, fi_volume_colour_sample) ----
    def colours(self, device=False):
        """the colour channels, (channels, num_voxels) float32, x fastest within a channel"""
        a, p = _cloud_out("cuda" if device else None, (self.channels, self.num_voxels), np.float32)
        check(_capi.lib().fi_volume_colour_copy(self._h, p, None, FI_DEVICE if device else FI_HOST))
        return a

    def colour_weight(self, device=False):
        """the colour weights, (num_voxels,) float32, x fastest"""
        a, p = _cloud_out("cuda" if device else None, (self.num_voxels,), np.float32)
        check(_capi.lib().fi_volume_colour_copy(self._h, None, p, FI_DEVICE if device else FI_HOST))
        return a

    def load_colours(self, colour, colour_weight):
        """sets the channels ((channels, num_voxels) values) and the colour weights (num_voxels values): resumes a fusion"""
        a, am, ak = _buf(colour)
        w, wm, wk = _buf(colour_weight)
        if _count(ak) != self.channels * self.num_voxels or _count(wk) != self.num_voxels:
            raise ValueError("colour must hold %d x %d values and colour_weight %d" % (self.channels, self.num_voxels, self.num_voxels))
        check(_capi.lib().fi_volume_colour_load(self._h, a, w, _same_memory(am, wm)))
        return self

    def sample_colours(self, positions, min_weight=0.0, valid=False):
        """The colour (n, channels) float32 at `positions` (n, 3) in lattice coordinates: the average of the corners of the
        point's cell that carry a colour (colour weight > 0 and >= min_weight) under the trilinear weights; NaN where none
        does or the point lies outside the lattice.  valid=True: also the (n,) booleans of that.
        vol.sample_colours(mesh.vertices) colours the vertices of iso_surface's or dual_contour's mesh.  numpy in, numpy out;
        a torch tensor on the GPU in, tensors on that GPU out."""
        p, mem, keep = _buf(positions)
        if _count(keep) % 3:
            raise ValueError("positions are (n, 3) (got %d values)" % _count(keep))
        n = _count(keep) // 3
        dev = keep.device if mem == FI_DEVICE else None
        col, cp = _cloud_out(dev, (n, self.channels), np.float32)
        val, vp = _cloud_out(dev, (n,), np.uint8) if valid else (None, None)
        check(_capi.lib().fi_volume_colour_sample(self._h, float(min_weight), n, p if n else None, cp, vp, mem))
        return (col, _as_mask(val)) if valid else col

    def colour_constraints(self, min_weight=0.0, device=False):
        """(positions (n, 3), colours (n, channels), weights (n,)) float32 of the voxels that carry a colour (colour weight > 0
        and >= min_weight) in ascending index; weights are Wc / max_weight.  A channel completed over the lattice by a solve:
        field.add_points(w, ValueKernel.kLinearInterpolation, 0.0, GradientKernel.kNearestNeighbor, positions,
        values=colours[:, k], point_weights=weights)."""
        n = C.c_long(0)
        check(_capi.lib().fi_volume_colour_constraints(self._h, float(min_weight), C.byref(n), None, None, None, FI_HOST))
        dev = "cuda" if device else None
        pos, pp = _cloud_out(dev, (n.value, 3), np.float32)
        col, pc = _cloud_out(dev, (n.value, self.channels), np.float32)
        wgt, pw = _cloud_out(dev, (n.value,), np.float32)
        if n.value:
            check(_capi.lib().fi_volume_colour_constraints(self._h, float(min_weight), C.byref(n), pp, pc, pw,
                                                           FI_DEVICE if device else FI_HOST))
        return pos, col, wgt

    def constraints(self, min_weight=0.0, device=False):
        """(positions (n, 3), values (n,), weights (n,)) float32 of the band: the voxels with weight >= min_weight, weight > 0
        and |tsdf| < 1 in ascending index; values are tsdf * truncation, weights W / max_weight."""
        n = C.c_long(0)
        check(_capi.lib().fi_volume_constraints(self._h, float(min_weight), C.byref(n), None, None, None, FI_HOST))
        dev = "cuda" if device else None
        pos, pp = _cloud_out(dev, (n.value, 3), np.float32)
        val, pv = _cloud_out(dev, (n.value,), np.float32)
        wgt, pw = _cloud_out(dev, (n.value,), np.float32)
        if n.value:
            check(_capi.lib().fi_volume_constraints(self._h, float(min_weight), C.byref(n), pp, pv, pw, FI_DEVICE if device else FI_HOST))
        return pos, val, wgt


    # ---- rays and images of the volume (include/fi_hip.h fi_volume_raycast, fi_volume_render) ----
    def raycast(self, origins, directions, iso=0.0, step=1.0, refine=4, side="front", min_weight=0.0, t_min=0.0, t_max=math.inf,
                positions=False, normals=False):
        """raycast_field against the volume's tsdf under its weights, both read in place: a sample counts only where every
        corner of its cell has weight > 0 and >= min_weight; iso=0 is the surface (tsdf is in units of `truncation`, the
        rays' t is not)."""
        opt = _march_options(iso, step, refine, side, min_weight)

        def call(n, o, d, tp, pp, np_, sp, mem):
            return _capi.lib().fi_volume_raycast(self._h, C.byref(opt), n, o, d, float(t_min), float(t_max), tp, pp, np_, sp, mem)
        return _march_rays(call, 3, origins, directions, positions, normals)

    def render(self, camera, step=1.0, refine=4, min_weight=0.0, positions=False, normals=False, incidence=False, device=False,
               colours=False, colour_min_weight=0.0):
        """The depth image (height, width) float32 of the volume's surface (tsdf = 0, front crossings) seen by `camera`, in
        the camera's own kind; +inf where a pixel's ray meets none.  With positions / normals / incidence also the hit points
        (h w, 3), the unit gradients (h w, 3) and the incidences (h w,) in depth_to_points' layout and conventions, so that
        integrate() can take the image and its incidences as they are.  colours=True (a volume with channels) appends the
        colour image (h w, channels): sample_colours(hit points, colour_min_weight), NaN where a pixel has no hit.  numpy
        arrays, or torch tensors with device=True."""
        opt = _march_options(0.0, step, refine, "front", min_weight)
        if not colours:
            def call(cam, dp, pp, np_, ip, mem):
                return _capi.lib().fi_volume_render(self._h, C.byref(opt), cam, dp, pp, np_, ip, mem)
            return _march_image(call, camera, positions, normals, incidence, device)
        col, cp = _cloud_out("cuda" if device else None, (camera.width * camera.height, self.channels), np.float32)

        def call(cam, dp, pp, np_, ip, mem):
            return _capi.lib().fi_volume_render_colour(self._h, C.byref(opt), cam, float(colour_min_weight), dp, pp, np_, ip, cp, mem)
        out = _march_image(call, camera, positions, normals, incidence, device)
        return (out if isinstance(out, tuple) else (out,)) + (col,)

    def track(self, camera, depth, rounds=2, max_jump=math.inf, max_distance=None, **register_keywords):
        """Refines the pose of `camera` from the depth image it took, against the surface the volume holds (frame-to-model
        tracking): each round renders the volume at the current pose with positions and normals, unprojects `depth` under
        the same pose (depth_to_points, max_jump), and lays the unprojected points over the rendered ones with
        register_points(mode="plane", target_normals=the rendered normals, max_distance=the volume's truncation by default,
        **register_keywords).  With G the guessed pose and T that transform, the new pose is G T^-1, composed in float64 and
        rounded to float32 once per round.  -> (Camera, dict): the last registration's dict plus "correction" (4, 4)
        float64, the product of the rounds' transforms, and "rendered" / "unprojected", the points of each round.  Every
        array stays on the device when `depth` is a device tensor."""
        device = hasattr(depth, "data_ptr") and depth.is_cuda
        max_distance = self.truncation if max_distance is None else max_distance
        total, rendered, unprojected, last = np.eye(4), [], [], {}
        for _ in range(int(rounds)):
            _, pos, nrm = self.render(camera, positions=True, normals=True, device=device)
            hit = pos[:, 0] == pos[:, 0]                 # (a pixel without a hit has a NaN position)
            src, = depth_to_points(camera, depth, max_jump, normals=False, incidence=False, valid=False, compact=True)
            last = register_points(src, pos[hit], nrm[hit], mode="plane", max_distance=max_distance, **register_keywords)
            G = np.eye(4)
            G[:3] = camera.pose.astype(np.float64)
            G = G @ np.linalg.inv(last["transform"])
            total = last["transform"] @ total
            camera = Camera(G[:3], camera.fx, camera.fy, camera.cx, camera.cy, camera.width, camera.height, camera.kind)
            rendered.append(int(hit.sum()))
            unprojected.append(int(src.shape[0]))
        return camera, dict(last, correction=total, rendered=rendered, unprojected=unprojected)


# ---- rays and images of a lattice field (include/fi_hip.h fi_field_raycast, fi_field_render) -----------------

def _march_options(iso, step, refine, side, min_weight):
    if side not in _capi.FI_MARCH:
        raise ValueError("side is 'front', 'back' or 'either', not %r" % (side,))
    return _capi.FiMarchOptions(float(iso), float(step), float(min_weight), int(refine), _capi.FI_MARCH[side])


def _march_rays(call, ndim, origins, directions, positions, normals, other_memory=()):
    """Shared body of the field raycasts: call(n, origins, directions, t, positions, normals, side, memory) -> (t (n,)
    float32, side (n,) int8[, positions (n, ndim)][, normals (n, ndim)]) where the rays live"""
    o, omem, okeep = _buf(origins)
    d, dmem, dkeep = _buf(directions)
    if _count(okeep) % ndim or _count(okeep) != _count(dkeep):
        raise ValueError("origins and directions are (n, %d) each (got %d and %d values)" % (ndim, _count(okeep), _count(dkeep)))
    n = _count(okeep) // ndim
    mem = _same_memory(omem, dmem, *other_memory)
    dev = okeep.device if mem == FI_DEVICE else None
    t, tp = _cloud_out(dev, (n,), np.float32)
    sd, sp = _cloud_out(dev, (n,), np.int8)
    pos, pp = _cloud_out(dev, (n, ndim), np.float32) if positions else (None, None)
    nrm, np_ = _cloud_out(dev, (n, ndim), np.float32) if normals else (None, None)
    if n:   # (an empty array has no storage to point at)
        check(call(n, o, d, tp, pp, np_, sp, mem))
    return tuple(a for a in (t, sd, pos, nrm) if a is not None)


def _march_image(call, camera, positions, normals, incidence, device, like=None):
    """Shared body of the field renders: call(camera, depth, positions, normals, incidence, memory) -> depth (h, w)[,
    positions (h w, 3)][, normals (h w, 3)][, incidence (h w,)]: numpy, or torch with device=True"""
    n = camera.width * camera.height
    dev = ("cuda" if like is None else like.device) if device else None
    depth, dp = _cloud_out(dev, (n,), np.float32)
    pos, pp = _cloud_out(dev, (n, 3), np.float32) if positions else (None, None)
    nrm, np_ = _cloud_out(dev, (n, 3), np.float32) if normals else (None, None)
    inc, ip = _cloud_out(dev, (n,), np.float32) if incidence else (None, None)
    cam = camera._c()
    check(call(C.byref(cam), dp, pp, np_, ip, FI_DEVICE if device else FI_HOST))
    out = tuple(a for a in (depth.reshape(camera.height, camera.width), pos, nrm, inc) if a is not None)
    return out if len(out) > 1 else out[0]


def raycast_field(field, sizes, origins, directions, iso=0.0, step=1.0, refine=4, side="front", weight=None, min_weight=0.0,
                  t_min=0.0, t_max=math.inf, positions=False, normals=False):
    """Rays against the iso-level of a lattice field (flat, fp32, x fastest, 2-D or 3-D), marched on the device through its
    trilinear interpolant: ray i is origins[i] + t directions[i] (n x ndim each, directions not normalised, t in units of the
    direction) with t_min <= t <= t_max.  The ray is clipped to the lattice's box and sampled every `step` lattice units; the
    first two consecutive samples that `iso` separates are refined by `refine` (0 .. 16) bisections and one linear
    interpolation.  side: "front" takes crossings from outside (f >= iso) to inside (f < iso, as iso_surface decides it),
    "back" the opposite ones, "either" the first of both.  weight (optional, the field's shape) with min_weight masks the
    field: a sample counts only where every corner of its cell has weight > 0 and >= min_weight.  -> (t (n,) float32, side
    (n,) int8: +1 front, -1 back, 0 none), with positions / normals also the hit points (n, ndim) and the field's unit
    gradients there (towards increasing f).  No crossing: +inf, NaN position, zero normal; a ray with a non-finite origin or
    direction, or a zero direction: NaN.  Two crossings inside one step, and features thinner than `step`, can be missed.
    numpy in, numpy out; torch CUDA tensors in (field, rays and weight alike), tensors out (include/fi_hip.h
    fi_field_raycast)."""
    sizes = [int(s) for s in sizes]
    opt = _march_options(iso, step, refine, side, min_weight)
    f, fmem, fkeep = _buf(field)
    w, wmem, wkeep = _buf(weight)
    total = int(np.prod(sizes))
    if _count(fkeep) != total or (wkeep is not None and _count(wkeep) != total):
        raise ValueError("field and weight hold %d values each for sizes %r" % (total, sizes))
    sz = (C.c_int * len(sizes))(*sizes)

    def call(n, o, d, tp, pp, np_, sp, mem):
        return _capi.lib().fi_field_raycast(f, w, len(sizes), sz, C.byref(opt), n, o, d, float(t_min), float(t_max), tp, pp, np_, sp, mem)
    return _march_rays(call, len(sizes), origins, directions, positions, normals, [fmem, wmem])


def render_field(field, sizes, camera, iso=0.0, step=1.0, refine=4, side="front", weight=None, min_weight=0.0, positions=False,
                 normals=False, incidence=False):
    """The depth image (height, width) float32 of the iso-level of a 3-D lattice field seen by `camera` (raycast_field along
    the pixels' rays, over t >= 0), in the camera's own kind; +inf where a pixel's ray meets no crossing.  positions /
    normals / incidence: as DepthVolume.render.  numpy in, numpy out; a torch CUDA field (and weight) in, tensors out
    (include/fi_hip.h fi_field_render)."""
    sizes = [int(s) for s in sizes]
    if len(sizes) != 3:
        raise ValueError("render_field needs a 3-D field")
    opt = _march_options(iso, step, refine, side, min_weight)
    f, fmem, fkeep = _buf(field)
    w, wmem, wkeep = _buf(weight)
    total = int(np.prod(sizes))
    if _count(fkeep) != total or (wkeep is not None and _count(wkeep) != total):
        raise ValueError("field and weight hold %d values each for sizes %r" % (total, sizes))
    sz = (C.c_int * 3)(*sizes)
    device = _same_memory(fmem, wmem) == FI_DEVICE

    def call(cam, dp, pp, np_, ip, mem):
        return _capi.lib().fi_field_render(f, w, sz, C.byref(opt), cam, dp, pp, np_, ip, mem)
    return _march_image(call, camera, positions, normals, incidence, device, fkeep if device else None)


def sdf_from_depth(sizes, weights, cameras, depths, truncation, incidences=None, min_incidence=0.5, max_weight=64.0, dtype="f32"):
    """A signed distance problem from depth images: a DepthVolume over `sizes` fuses them, the model rows of `weights` and the
    volume's band (value rows of weight weights.data_pos) make the field -> (field, volume), ready for field.solve_cg().
    The rows' point weights are W / max_weight: choose max_weight near the number of views that see a surface point at
    min_incidence or better (about 4 of 14 views all around an object), or raise weights.data_pos -- with weights of a few
    hundredths the smoothness rows win and the surface moves by cells."""
    volume = DepthVolume(sizes, truncation, max_weight)
    volume.integrate(cameras, depths, incidences, min_incidence=min_incidence)
    field = LatticeField(sizes, dtype=dtype)
    field.add_field_constraints(weights)
    field.add_volume(volume, weights.data_pos)
    return field, volume


def solve_sparse_linear_with_guess(field, guess, max_iterations=0, error_tolerance=0.0):
    """solve_sparse_linear_with_guess (sparse_linear.cpp:186-212).  0 => defaults (2N iterations, fp32 eps)."""
    res = field.solve_cg(guess, max_iterations, error_tolerance)
    return None if res is None else res[0]


def jacobi_iterations(field, guess, num_iterations, weight):
    """jacobi_iterations (sparse_linear.cpp:214-241); num_iterations <= 0 returns the guess (:220)."""
    if num_iterations <= 0:
        return np.array(guess, np.float32, copy=True) if not hasattr(guess, "data_ptr") else guess.clone()
    return field.jacobi(guess, num_iterations, weight)


def generate_error_map(field, solution):
    """generate_error_map(field.eq.triplets, solution, field.eq.rhs) (field_interpolation.cpp:402-429); the rows
    live on the device, so the field stands in for its triplet list."""
    return field.error_map(solution)


def solve_tiled_with_guess(field, guess, sizes, options):
    """solve_tiled_with_guess (sparse_linear.cpp:392-443): wrong guess length -> None (:402-405); optional tile
    pre-pass (options.tile, :415-425), then optional CG (options.cg, :427-440)."""
    n = int(np.prod(sizes))
    glen = guess.numel() if hasattr(guess, "numel") else np.asarray(guess).size
    if glen != n:
        return None
    if options.tile:
        guess = field.tile_pass(guess, options.tile_size)
    if not options.cg:
        return guess if options.tile else np.array(guess, np.float32, copy=True)
    res = field.solve_cg(guess, options.max_iterations, options.error_tolerance)
    return None if res is None else res[0]


def solve_sparse_linear_exact(field, num_columns=None, tolerance=1e-12, max_iterations=0):
    """Stands in for solve_sparse_linear_exact (sparse_linear.cpp:154-184): the reference factorises AtA
    (sparse Cholesky, double).  On the GPU the same system is iterated to `tolerance` in fp64; create the
    field with dtype="f64" for this.  Returns None where the reference returns {}: an unknown without any equation (the
    zero pivot that stops the factorisation) or a solver breakdown.  A well-posed system whose attainable residual
    (about eps * kappa) stays above `tolerance` returns its best iterate with a warning -- the factorisation would
    still answer."""
    import warnings
    if field.dtype != "f64":
        raise ValueError("solve_sparse_linear_exact needs a dtype='f64' field")
    field._ready()
    if not (field.diag() > 0).all():
        return None
    if max_iterations <= 0:
        # CG in floating point can need several times N steps on these kappa ~ side^4 systems
        max_iterations = max(2000, 20 * field.num_unknowns)
    res = field.solve_cg(None, max_iterations, tolerance)
    if res is None:
        return None
    x, it, rel = res
    if not (rel <= tolerance * 1.0001):
        warnings.warn("solve_sparse_linear_exact: relative residual %g after %d iterations (asked for %g)" % (rel, it, tolerance))
    return x


def upscale_field(field, small_sizes, large_sizes):
    """upscale_field (field_interpolation.cpp:431-485)."""
    src, mem, keep = _buf(field)
    ss = (C.c_int * len(small_sizes))(*[int(s) for s in small_sizes])
    ls = (C.c_int * len(large_sizes))(*[int(s) for s in large_sizes])
    n = int(np.prod(large_sizes))
    if mem == FI_DEVICE:
        import torch
        out = torch.empty(n, dtype=torch.float32, device=keep.device)
        o = C.c_void_p(out.data_ptr())
    else:
        out = np.empty(n, np.float32)
        o = C.c_void_p(out.ctypes.data)
    check(_capi.lib().fi_upscale_field(src, len(small_sizes), ss, ls, o, mem))
    return out


def iso_surface(field, sizes, iso=0.0, normals=True, largest=None, min_size=None, parts=False, simplify=None, smooth=None):
    """The iso-contour (2-D) / iso-surface (3-D) f = iso of a whole lattice field (numpy array or torch CUDA tensor, x
    fastest), e.g. the output of upscale_field.  -> IsoMesh.  largest, min_size, parts, simplify, smooth: as
    LatticeField.iso_surface's."""
    src, mem, _keep = _buf(field)
    sz = (C.c_int * len(sizes))(*[int(s) for s in sizes])
    h = C.c_void_p()
    check(_capi.lib().fi_iso_extract_field(src, len(sizes), sz, float(iso), mem, C.byref(h)))
    return _finish_mesh(h, len(sizes), normals, largest, min_size, parts, simplify, smooth)


def dual_contour(field, sizes, iso=0.0, gradients=None, normals=True, largest=None, min_size=None, parts=False, simplify=None,
                 smooth=None):
    """LatticeField.dual_contour of a whole lattice field (numpy array or torch CUDA tensor, x fastest); gradients:
    (prod(sizes), ndim) in the same memory, or None.  -> IsoMesh.  largest, min_size, parts, simplify, smooth:
    as LatticeField.iso_surface's."""
    src, mem, _keep = _buf(field)
    g, gmem, _kg = _buf(gradients)
    mem = _same_memory(mem, gmem)
    sz = (C.c_int * len(sizes))(*[int(s) for s in sizes])
    h = C.c_void_p()
    check(_capi.lib().fi_dual_contour_field(src, g, len(sizes), sz, float(iso), mem, C.byref(h)))
    return _finish_mesh(h, len(sizes), normals, largest, min_size, parts, simplify, smooth)


def redistance(field, sizes, iso=0.0, method="iso", max_distance=math.inf):
    """LatticeField.redistance of a whole lattice field (numpy array or torch CUDA tensor, x fastest): the signed distances,
    flat, where the field lives"""
    src, mem, _keep = _buf(field)
    sz = (C.c_int * len(sizes))(*[int(s) for s in sizes])
    m = _surface_method(method)

    def call(d, i, h, mm):
        return _capi.lib().fi_redistance_field(src, len(sizes), sz, float(iso), m, float(max_distance), d, i, h, mm)
    return _redistance(call, int(np.prod(sizes)), False, mem == FI_DEVICE, len(sizes))


def sample_field(field, sizes, positions, gradients=False, cubic=False, fill=float("nan")):
    """LatticeField.sample of a whole lattice field (numpy array or torch CUDA tensor, x fastest), e.g. the output of
    upscale_field; field and positions live in the same memory."""
    src, mem, _keep = _buf(field)
    sz = (C.c_int * len(sizes))(*[int(s) for s in sizes])

    def call(n, p, mode, fl, v, g, m):
        return _capi.lib().fi_sample_field(src, len(sizes), sz, n, p, mode, fl, v, g, m)
    return _sample(call, len(sizes), positions, [mem], gradients, cubic, fill)
