"""The point-set operations that exist on two faces of the C ABI -- fi_<op>(context, ...) over a context's data points and
fi_points_<op>(point set, ...) over a set of its own -- as a table for the tests that hold the two faces together
(test_point_faces.py, test_gpu_point_faces.py): every operation's arguments after the handle, by name, with values that pass
its checks for a set of m points in D dimensions and n queries."""
import ctypes as C
import math

import numpy as np

from field_interpolation_amd import _capi


def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class Buffers:
    """Host buffers large enough for every operation over m points and n queries in D dimensions, and for a distance
    field of `lattice` -- a context's own lattice where a context is called: that is what it writes"""

    def __init__(self, D, m, n, lattice):
        self.D, self.m, self.n = D, m, n
        rows = max(m, n, 1)
        self.queries = np.ones((max(n, 1), D), np.float32)
        self.f = [np.empty((rows, D), np.float32) for _ in range(3)]
        self.idx = np.empty(rows * 32, np.int64)
        self.wide = np.empty(rows * 32, np.float32)
        self.i32 = np.empty(rows, np.int32)
        self.u8 = [np.empty(rows, np.uint8) for _ in range(2)]
        self.sizes = (C.c_int * D)(*lattice)
        total = int(np.prod(list(self.sizes)))
        self.field = np.empty(total, np.float32)
        self.field_idx = np.empty(total, np.int64)
        self.outlier_stats = _capi.FiOutlierStats()
        self.cluster_stats = _capi.FiClusterStats()
        self.kept = C.c_long(0)


def _arguments(b):
    q, f, u8 = ptr(b.queries), [ptr(a) for a in b.f], [ptr(a) for a in b.u8]
    return {
        "nearest": [("n", b.n), ("queries", q), ("max_distance", math.inf), ("distances", ptr(b.wide)), ("indices", ptr(b.idx)),
                    ("memory", 0)],
        # (`sizes` goes to the point-set face alone: a context brings its lattice)
        "distance_field": [("sizes", b.sizes), ("max_distance", math.inf), ("out", ptr(b.field)), ("indices", ptr(b.field_idx)),
                           ("memory", 0)],
        "knn": [("n", b.n), ("queries", q), ("k", 8), ("max_distance", math.inf), ("distances", ptr(b.wide)), ("indices", ptr(b.idx)),
                ("memory", 0)],
        "estimate_normals": [("k", 8), ("max_distance", math.inf), ("orient", 0), ("guides", None), ("num_guides", 0), ("normals", f[0]),
                             ("variation", ptr(b.wide)), ("memory", 0)],
        "orient_normals": [("k", 8), ("max_distance", math.inf), ("anchor", 0), ("guides", None), ("num_guides", 0), ("normals", f[0]),
                           ("components", ptr(b.idx)), ("memory", 0)],
        "mls_project": [("n", b.n), ("queries", q), ("k", 8), ("radius", 2.0), ("degree", 2), ("max_move", math.inf),
                        ("guide_normals", None), ("positions", f[0]), ("normals", f[1]), ("curvature", ptr(b.wide)), ("order", u8[0]),
                        ("memory", 0)],
        "radius_count": [("n", b.n), ("queries", q), ("radius", 2.0), ("limit", 100), ("counts", ptr(b.i32)), ("memory", 0)],
        "neighbour_distances": [("k", 8), ("max_distance", math.inf), ("mean", f[0]), ("kth", f[1]), ("counts", ptr(b.i32)), ("memory", 0)],
        "outliers_statistical": [("k", 8), ("max_distance", math.inf), ("std_ratio", 2.0), ("keep", u8[0]),
                                 ("stats", C.byref(b.outlier_stats)), ("memory", 0)],
        "outliers_radius": [("radius", 2.0), ("min_neighbours", 2), ("keep", u8[0]), ("num_kept", C.byref(b.kept)), ("memory", 0)],
        "cluster": [("eps", 1.5), ("min_points", 2), ("labels", ptr(b.i32)), ("core", u8[0]), ("stats", C.byref(b.cluster_stats)),
                    ("memory", 0)],
    }


OPS = tuple(_arguments(Buffers(2, 1, 1, [1, 1])))
CONTEXT_FACE, SET_FACE = "fi_", "fi_points_"


def call(face, op, handle, b, **changed):
    """fi_<op> or fi_points_<op> on `handle` with the table's arguments, those named in `changed` replaced
    -> (status code, fi_last_error's text)"""
    table = _arguments(b)[op]
    unknown = set(changed) - {name for name, _ in table}
    assert not unknown, (op, unknown)
    args = [changed.get(name, value) for name, value in table if not (name == "sizes" and face == CONTEXT_FACE)]
    lib = _capi.lib()
    code = getattr(lib, face + op)(handle, *args)
    return code, lib.fi_last_error().decode()
