"""The C++ side of the sphere and cylinder segmentation through libfield_interpolation.so: segment_shape and segment_shapes
(include/field_interpolation/gpu_field.hpp) must give the C ABI's bytes -- the program checks that itself, with host and with
device pointers -- and the Python API's on the same cloud.  tests/cxx/test_shape.cpp is the program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import shape_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_shape")
NEW = ["fi_shape_fit", "fi_shapes_segment"]
INTS = ("found", "refits", "inliers", "candidates", "trials")


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_shape.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_shape_compiles_and_links():
    assert os.path.exists(os.path.join(PKG, "libfi_hip.so")), "libfi_hip.so is not built"
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::segment_shape(" in syms and "field_interpolation::segment_shapes(" in syms
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "libfi_hip.so")], text=True).split()
    for name in NEW:
        assert name in exported, name


def test_struct_mirrors_match_the_header():
    from field_interpolation_amd import _capi
    # int, 4 floats, (pad), long, double, int, (pad), unsigned long long
    assert C.sizeof(_capi.FiShapeOptions) == 4 + 4 * 4 + 4 + 8 + 8 + 8 + 8
    # 3 ints, (pad), 3 longs, 3 + 3 + 1 + 2 + 1 doubles
    assert C.sizeof(_capi.FiShapeModel) == 3 * 4 + 4 + 3 * C.sizeof(C.c_long) + 10 * 8
    assert [f for f, _ in _capi.FiShapeOptions._fields_] == ["kind", "threshold", "r_min", "r_max", "normal_cos", "max_trials", "confidence",
                                                             "refine", "seed"]
    assert [f for f, _ in _capi.FiShapeModel._fields_] == ["found", "kind", "refits", "inliers", "candidates", "trials", "center", "axis",
                                                           "radius", "extent", "rms"]
    header = open(os.path.join(ROOT, "include", "fi_hip.h")).read()
    for struct, mirror in (("fi_shape_options", _capi.FiShapeOptions), ("fi_shape_model", _capi.FiShapeModel)):
        body = header[header.index("typedef struct %s {" % struct):header.index("} %s;" % struct)]
        at = [body.index(name) for name, _ in mirror._fields_]
        assert at == sorted(at), struct
    assert "fi_shape_fit" in _capi.SYMBOLS and "fi_shapes_segment" in _capi.SYMBOLS
    for name, value in (("FI_SHAPE_SPHERE", _capi.FI_SHAPE["sphere"]), ("FI_SHAPE_CYLINDER", _capi.FI_SHAPE["cylinder"]), ("FI_SHAPE_BATCH", 1024)):
        assert "#define %s" % name in header and int(header.split("#define %s" % name)[1].split()[0]) == value, name


def _read(path, dtypes):
    out = []
    with open(path, "rb") as f:
        for dtype in dtypes:
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


def _same(got, want, ref, cylinder):
    for key in INTS:
        assert getattr(got, key) == int(want[key]) == ref[key], key
    assert got.kind == ref["kind"]
    assert np.float64(got.center[:]).tobytes() == want["center"].tobytes() == ref["center"].tobytes()
    assert np.float64([got.radius, got.rms]).tobytes() == np.float64([want["radius"], want["rms"]]).tobytes()
    assert np.float64([got.radius, got.rms]).tobytes() == np.float64([ref["radius"], ref["rms"]]).tobytes()
    assert np.float64(got.axis[:] + got.extent[:]).tobytes() == np.concatenate([ref["axis"], ref["extent"]]).tobytes()
    if cylinder:
        assert np.concatenate([want["axis"], want["extent"]]).tobytes() == np.concatenate([ref["axis"], ref["extent"]]).tobytes()


@pytest.mark.gpu
def test_cxx_shape_equals_python(tmp_path):
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    exe = _build()
    pos, nrm, _planted = SR.planted_cylinder(6)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + nrm.tobytes())
    res = tmp_path / "shape_out.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all shape checks passed" in r.stdout
    raw, inliers, sphere, labels, rows = _read(res, (np.uint8, np.uint8, np.uint8, np.int32, np.uint8))
    want, want_inl = fi.segment_cylinder(pos, nrm, 0.05, 0.1, 2.0)
    ref, ref_inl = SR.fit(pos, SR.CYLINDER, 0.05, 0.1, 2.0, normals=nrm)
    assert np.array_equal(inliers.view(np.bool_), want_inl) and np.array_equal(inliers, ref_inl)
    size = C.sizeof(_capi.FiShapeModel)
    assert len(raw) == size == len(sphere) and len(rows) % size == 0 and len(rows) >= size
    for buf in (raw, rows[:size]):
        _same(_capi.FiShapeModel.from_buffer_copy(buf.tobytes()), want, ref, True)
    want, _ = fi.segment_sphere(pos, 0.05, 0.5)
    ref, _ = SR.fit(pos, SR.SPHERE, 0.05, 0.5)
    _same(_capi.FiShapeModel.from_buffer_copy(sphere.tobytes()), want, ref, False)
    got_labels, models = fi.segment_shapes(pos, "cylinder", 0.05, 3, min_inliers=400, normals=nrm, r_min=0.1, r_max=2.0)
    assert np.array_equal(labels, got_labels) and len(models) == len(rows) // size
