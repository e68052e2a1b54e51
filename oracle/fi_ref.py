"""ctypes front end of oracle/_ref/libfi_ref.so: the REFERENCE's own assembly half (field_interpolation.cpp as it stands,
add_equation and operator<< from the head of sparse_linear.cpp), compiled by oracle/Makefile where the reference's sources
are at hand, behind the C ABI of fi_ref_capi.cpp.

TEST INFRASTRUCTURE ONLY.  Same method names as fi_oracle.LatticeField, so a test can drive both with one function.  A
failed reference check (where the reference would abort) raises RefCheckFailed.  There are no solvers here: they need Eigen.
"""
import ctypes as C
import os

import numpy as np

from .fi_oracle import Weights  # same members, same order  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(_HERE, "_ref", "libfi_ref.so")
_LIB = None


class RefCheckFailed(RuntimeError):
    pass


def reference_dir():
    """Where build() looks for the reference's sources."""
    return os.path.abspath(os.environ.get("FI_REFERENCE_DIR") or os.path.join(os.path.dirname(os.path.dirname(_HERE)), "reference"))


def reference_present():
    return os.path.isfile(os.path.join(reference_dir(), "field_interpolation", "field_interpolation.cpp"))


def available():
    return os.path.exists(SO)


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(SO, mode=C.RTLD_LOCAL)   # its C++ symbols carry the names the drop-in library exports too
        fp, ip, vp, lp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_long)
        L.fir_last_error.restype = C.c_char_p
        L.fir_field_new.argtypes = [C.c_int, ip, C.POINTER(vp)]
        L.fir_field_free.argtypes = [vp]
        L.fir_counts.argtypes = [vp, lp, lp]
        L.fir_get.argtypes = [vp, ip, ip, fp, fp]
        L.fir_add_equation.argtypes = [vp, C.c_float, C.c_float, C.c_int, ip, fp]
        L.fir_add_field_constraints.argtypes = [vp, C.POINTER(Weights)]
        L.fir_add_points.argtypes = [vp, C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, fp, fp, fp]
        L.fir_sdf_from_points.argtypes = [C.c_int, ip, C.POINTER(Weights), C.c_int, fp, fp, fp, C.POINTER(vp)]
        L.fir_add_value_constraint.argtypes = [vp, fp, C.c_float, C.c_float, ip]
        L.fir_add_value_constraint_nearest_neighbor.argtypes = [vp, fp, fp, C.c_float, C.c_float, ip]
        L.fir_add_gradient_constraint.argtypes = [vp, fp, fp, C.c_float, C.c_int, ip]
        L.fir_error_map.argtypes = [vp, C.c_long, fp, fp]
        L.fir_upscale_field.argtypes = [fp, C.c_int, ip, C.c_int, ip, C.c_long, fp]
        L.fir_print.argtypes = [vp, C.c_char_p, C.c_long, lp]
        _LIB = L
    return _LIB


def _check(status):
    if status != 0:
        msg = lib().fir_last_error().decode("utf-8", "replace")
        raise (RefCheckFailed if status == 1 else RuntimeError)(msg)


def _f(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


class LatticeField:
    """field_interpolation::LatticeField of the reference; `.get()` copies out `eq`."""

    def __init__(self, sizes, _handle=None):
        self.sizes = [int(s) for s in sizes]
        self._sz = np.asarray(self.sizes, dtype=np.int32)
        if _handle is None:
            _handle = C.c_void_p()
            _check(lib().fir_field_new(len(self.sizes), _i(self._sz), C.byref(_handle)))
        self._h = _handle

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.fir_field_free(self._h)
            self._h = None

    @property
    def num_unknowns(self):
        return int(np.prod(self.sizes)) if self.sizes else 1

    def _counts(self):
        nr, nt = C.c_long(0), C.c_long(0)
        _check(lib().fir_counts(self._h, C.byref(nr), C.byref(nt)))
        return nr.value, nt.value

    @property
    def num_rows(self):
        return self._counts()[0]

    @property
    def num_triplets(self):
        return self._counts()[1]

    def get(self):
        nr, nt = self._counts()
        rows, cols = np.empty(nt, np.int32), np.empty(nt, np.int32)
        vals, rhs = np.empty(nt, np.float32), np.empty(nr, np.float32)
        _check(lib().fir_get(self._h, _i(rows), _i(cols), _f(vals), _f(rhs)))
        return rows, cols, vals, rhs

    def add_equation(self, weight, rhs, pairs):
        cols = np.asarray([p[0] for p in pairs], np.int32)
        coef = np.asarray([p[1] for p in pairs], np.float32)
        _check(lib().fir_add_equation(self._h, weight, rhs, len(pairs), _i(cols), _f(coef)))

    def add_value_constraint(self, pos, value, weight):
        p, ok = _f32(np.atleast_1d(pos)), C.c_int(0)
        _check(lib().fir_add_value_constraint(self._h, _f(p), value, weight, C.byref(ok)))
        return bool(ok.value)

    def add_value_constraint_nearest_neighbor(self, pos, gradient, value, weight):
        p, g, ok = _f32(np.atleast_1d(pos)), _f32(np.atleast_1d(gradient)), C.c_int(0)
        _check(lib().fir_add_value_constraint_nearest_neighbor(self._h, _f(p), _f(g), value, weight, C.byref(ok)))
        return bool(ok.value)

    def add_gradient_constraint(self, pos, gradient, weight, kernel):
        p, g, ok = _f32(np.atleast_1d(pos)), _f32(np.atleast_1d(gradient)), C.c_int(0)
        _check(lib().fir_add_gradient_constraint(self._h, _f(p), _f(g), weight, kernel, C.byref(ok)))
        return bool(ok.value)

    def add_field_constraints(self, weights):
        _check(lib().fir_add_field_constraints(self._h, C.byref(weights)))

    def add_points(self, value_weight, value_kernel, gradient_weight, gradient_kernel, positions, normals=None,
                   point_weights=None):
        pos, nrm, pw = _f32(positions), _f32(normals), _f32(point_weights)
        n = pos.size // max(1, len(self.sizes))
        _check(lib().fir_add_points(self._h, value_weight, value_kernel, gradient_weight, gradient_kernel, n, _f(pos), _f(nrm),
                                    _f(pw)))

    def error_map(self, solution):
        sol = _f32(solution)
        out = np.empty_like(sol)
        _check(lib().fir_error_map(self._h, sol.size, _f(sol), _f(out)))
        return out

    def text(self):
        """What operator<< prints for `eq`."""
        need = C.c_long(0)
        _check(lib().fir_print(self._h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(max(1, need.value))
        _check(lib().fir_print(self._h, buf, need.value, C.byref(need)))
        return buf.raw[:need.value]


def sdf_from_points(sizes, weights, positions, normals=None, point_weights=None):
    sz = np.asarray(sizes, np.int32)
    pos, nrm, pw = _f32(positions), _f32(normals), _f32(point_weights)
    h = C.c_void_p()
    _check(lib().fir_sdf_from_points(len(sz), _i(sz), C.byref(weights), pos.size // len(sz), _f(pos), _f(nrm), _f(pw),
                                     C.byref(h)))
    return LatticeField(sizes, _handle=h)


def upscale_field(small, small_sizes, large_sizes):
    s = _f32(small)
    ss, ls = np.asarray(small_sizes, np.int32), np.asarray(large_sizes, np.int32)
    out = np.empty(int(np.prod(ls)), np.float32)
    _check(lib().fir_upscale_field(_f(s), len(ss), _i(ss), len(ls), _i(ls), out.size, _f(out)))
    return out
