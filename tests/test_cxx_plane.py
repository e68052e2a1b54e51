"""The C++ side of the plane segmentation through libfield_interpolation.so: segment_plane and segment_planes
(include/field_interpolation/gpu_field.hpp) must give the C ABI's bytes -- the program checks that itself, with host and with
device pointers -- and the Python API's on the same cloud.  tests/cxx/test_plane.cpp is the program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plane_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_plane")
NEW = ["fi_plane_fit", "fi_planes_segment"]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_plane.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_plane_compiles_and_links():
    assert os.path.exists(os.path.join(PKG, "libfi_hip.so")), "libfi_hip.so is not built"
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::segment_plane(" in syms and "field_interpolation::segment_planes(" in syms
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "libfi_hip.so")], text=True).split()
    for name in NEW:
        assert name in exported, name


def test_struct_mirrors_match_the_header():
    from field_interpolation_amd import _capi
    # float, long, double, int, unsigned long long, float[3], float: 8-byte alignment pads the float and the int
    assert C.sizeof(_capi.FiPlaneOptions) == 8 + 8 + 8 + 8 + 8 + 12 + 4
    assert C.sizeof(_capi.FiPlaneModel) == 2 * 4 + 3 * C.sizeof(C.c_long) + 5 * 8
    assert [f for f, _ in _capi.FiPlaneOptions._fields_] == ["threshold", "max_trials", "confidence", "refine", "seed", "axis", "min_cos"]
    assert [f for f, _ in _capi.FiPlaneModel._fields_] == ["found", "refits", "inliers", "candidates", "trials", "normal", "offset", "rms"]
    header = open(os.path.join(ROOT, "include", "fi_hip.h")).read()
    for struct, mirror in (("fi_plane_options", _capi.FiPlaneOptions), ("fi_plane_model", _capi.FiPlaneModel)):
        body = header[header.index("typedef struct %s {" % struct):header.index("} %s;" % struct)]
        at = [body.index(name) for name, _ in mirror._fields_]
        assert at == sorted(at), struct
    assert "fi_plane_fit" in _capi.SYMBOLS and "fi_planes_segment" in _capi.SYMBOLS


def _read(path, dtypes):
    out = []
    with open(path, "rb") as f:
        for dtype in dtypes:
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_plane_equals_python(tmp_path):
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    exe = _build()
    pos, _floor = PR.planted_cloud(6)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes())
    res = tmp_path / "plane_out.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all plane checks passed" in r.stdout
    raw, inliers, labels, rows = _read(res, (np.uint8, np.uint8, np.int32, np.uint8))
    want, want_inl = fi.segment_plane(pos, 0.15)
    ref, ref_inl = PR.fit(pos, 0.15)
    assert np.array_equal(inliers.view(np.bool_), want_inl) and np.array_equal(inliers, ref_inl)
    assert len(raw) == C.sizeof(_capi.FiPlaneModel) == len(rows)
    for buf in (raw, rows):
        got = _capi.FiPlaneModel.from_buffer_copy(buf.tobytes())
        for key in ("found", "refits", "inliers", "candidates", "trials"):
            assert getattr(got, key) == int(want[key]) == ref[key], key
        assert np.float64(got.normal[:]).tobytes() == want["normal"].tobytes() == ref["normal"].tobytes()
        assert np.float64([got.offset, got.rms]).tobytes() == np.float64([want["offset"], want["rms"]]).tobytes()
        assert np.float64([got.offset, got.rms]).tobytes() == np.float64([ref["offset"], ref["rms"]]).tobytes()
    assert np.array_equal(labels, fi.segment_planes(pos, 0.15, 3, min_inliers=400)[0])
