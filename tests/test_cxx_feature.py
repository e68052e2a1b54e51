"""The C++ side of the descriptors and their matching through libfield_interpolation.so: describe_points and match_features
(include/field_interpolation/gpu_field.hpp) must give the C ABI's bytes -- the program checks that itself, with host and with
device pointers -- and the Python API's and the restatement's on the same cloud.  tests/cxx/test_feature.cpp is the program."""
import os
import subprocess

import numpy as np
import pytest

import feature_reference as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_feature")


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_feature.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_feature_compiles_and_links():
    assert os.path.exists(os.path.join(PKG, "libfi_hip.so")), "libfi_hip.so is not built"
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::describe_points(" in syms and "field_interpolation::match_features(" in syms
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "libfi_hip.so")], text=True).split()
    for name in ("fi_points_describe", "fi_feature_match"):
        assert name in exported, name
    header = open(os.path.join(ROOT, "include", "fi_hip.h")).read()
    assert "#define FI_FEATURE_WIDTH %d" % FR.WIDTH in header and "#define FI_FEATURE_MAX_DIM 64" in header


def _read(path, dtypes):
    out = []
    with open(path, "rb") as f:
        for dtype in dtypes:
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_feature_equals_python(tmp_path):
    import field_interpolation_amd as fi
    exe = _build()
    rng = np.random.default_rng(3)
    n = 601
    x, y = rng.uniform(0, 12, n), rng.uniform(0, 12, n)
    pos = np.stack([x, y, np.sin(x) + 0.5 * np.cos(1.7 * y)], axis=1).astype(np.float32)
    nrm = np.stack([-np.cos(x), 0.85 * np.sin(1.7 * y), np.ones(n)], axis=1).astype(np.float32)
    nrm[::40] = 0.0                                                        # a few points without a descriptor
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(n).tobytes() + pos.tobytes() + nrm.tobytes())
    res = tmp_path / "feature_out.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all feature checks passed" in r.stdout
    feat, valid, idx, dist = _read(res, (np.float32, np.uint8, np.int64, np.float32))
    want, want_valid = fi.PointIndex(pos).describe(nrm, 16)
    ref, ref_valid = FR.describe(pos, nrm, 16)
    assert np.array_equal(valid.view(np.bool_), want_valid) and np.array_equal(valid, ref_valid) and not valid[::40].any()
    assert feat.tobytes() == want.tobytes() == ref.tobytes()
    na = n // 2
    want_idx, want_dist = fi.match_features(want[:na], want[na:], want_valid[:na], want_valid[na:], distances=True)
    ref_idx, ref_dist = FR.match(ref[:na], ref[na:], ref_valid[:na], ref_valid[na:])
    assert np.array_equal(idx, want_idx) and np.array_equal(idx, ref_idx)
    assert dist.tobytes() == want_dist.tobytes() == ref_dist.tobytes()
