"""The C++ side of the coarse alignment through libfield_interpolation.so: align_correspondences
(include/field_interpolation/gpu_field.hpp) must give the C ABI's bytes -- the program checks that itself, with host and with
device pointers -- and the Python API's and the restatement's on the same pairs.  tests/cxx/test_align.cpp is the program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import align_reference as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_align")


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_align.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_align_compiles_and_links():
    assert os.path.exists(os.path.join(PKG, "libfi_hip.so")), "libfi_hip.so is not built"
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::align_correspondences(" in syms
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "libfi_hip.so")], text=True).split()
    assert "fi_align_correspondences" in exported


def test_struct_mirrors_match_the_header():
    from field_interpolation_amd import _capi
    # float, float, long, double, unsigned long long; int (padded to 8), five longs, 16 + 1 doubles
    assert C.sizeof(_capi.FiAlignOptions) == 4 + 4 + 8 + 8 + 8
    assert C.sizeof(_capi.FiAlignment) == 8 + 5 * C.sizeof(C.c_long) + 17 * 8
    assert [f for f, _ in _capi.FiAlignOptions._fields_] == ["threshold", "similarity", "max_trials", "confidence", "seed"]
    assert [f for f, _ in _capi.FiAlignment._fields_] == ["found", "pairs", "live", "trials", "valid", "inliers", "transform", "rms"]
    header = open(os.path.join(ROOT, "include", "fi_hip.h")).read()
    for struct, mirror in (("fi_align_options", _capi.FiAlignOptions), ("fi_alignment", _capi.FiAlignment)):
        body = header[header.index("typedef struct %s {" % struct):header.index("} %s;" % struct)]
        at = [body.index(name) for name, _ in mirror._fields_]
        assert at == sorted(at), struct
    assert "#define FI_ALIGN_BATCH %d" % AR.BATCH in header
    assert "fi_align_correspondences" in _capi.SYMBOLS


def _read(path, dtypes):
    out = []
    with open(path, "rb") as f:
        for dtype in dtypes:
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_align_equals_python(tmp_path):
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    exe = _build()
    src, tgt, _, _ = AR.moved_pairs(6, 700, 0.4)
    rng = np.random.default_rng(2)
    si = rng.permutation(700).astype(np.int64)
    ti = si.copy()
    si[::50] = -1                                                          # a few pairs without a partner
    pairs = tmp_path / "pairs.bin"
    with open(pairs, "wb") as f:
        f.write(np.int32([700, 700, 700]).tobytes() + src.tobytes() + tgt.tobytes() + si.tobytes() + ti.tobytes())
    res = tmp_path / "align_out.bin"
    r = subprocess.run([exe, str(pairs), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all align checks passed" in r.stdout
    raw, inliers = _read(res, (np.uint8, np.uint8))
    want, want_inl = fi.align_correspondences(src, tgt, si, ti, 0.05)
    ref, ref_inl = AR.align(src, tgt, si, ti, 0.05)
    assert np.array_equal(inliers.view(np.bool_), want_inl) and np.array_equal(inliers, ref_inl)
    assert len(raw) == C.sizeof(_capi.FiAlignment)
    got = _capi.FiAlignment.from_buffer_copy(raw.tobytes())
    for key in ("found", "pairs", "live", "trials", "valid", "inliers"):
        assert getattr(got, key) == int(want[key]) == int(ref[key]), key
    assert np.float64(got.transform[:]).tobytes() == want["transform"].tobytes() == ref["transform"].tobytes()
    assert np.float64([got.rms]).tobytes() == np.float64([want["rms"]]).tobytes() == np.float64([ref["rms"]]).tobytes()
    assert want["live"] == 686 and want["inliers"] > 137      # (a fifth of the live pairs; two fifths follow the motion)
