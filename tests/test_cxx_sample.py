"""GpuLatticeField::sample (include/field_interpolation/gpu_field.hpp) through libfield_interpolation.so: the C++ program
tests/cxx/test_sample.cpp solves a 3-D SDF, samples the solution in place at the data points and checks the
device-pointer paths of fi_sample / fi_sample_field against it; the results must equal the numpy oracle on the solution
the program returns, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import sample_reference as R
from util import sphere_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_sample")
SIZES = [40, 36, 32]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_sample.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_sample_compiles_and_links():
    if not os.path.exists(os.path.join(PKG, "libfi_hip.so")):
        pytest.skip("libfi_hip.so not built")
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::GpuLatticeField::sample" in syms


def _read(path):
    out = []
    with open(path, "rb") as f:
        for _ in range(5):
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * 4), np.float32))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


@pytest.mark.gpu
def test_cxx_sample_equals_the_oracle(tmp_path):
    exe = _build()
    pos, nrm = sphere_points(np.random.default_rng(6), SIZES, 2500)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + nrm.tobytes())
    res = tmp_path / "samples.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all sample checks passed" in r.stdout
    x, v, g, cv, cg = _read(res)
    q = np.concatenate([pos, np.array([[-1, 1, 1], [1, 36, 1], [1, 1, np.nan]], np.float32)])
    for cubic, got_v, got_g in ((False, v, g), (True, cv, cg)):
        want_v, want_g = R.sample(x, SIZES, q, cubic=cubic, gradients=True)
        assert np.array_equal(_bits(got_v), _bits(want_v))
        assert np.array_equal(_bits(got_g), _bits(want_g))
    # the data points sit near the zero set of the SDF
    assert np.median(np.abs(v[:len(pos)])) < 0.3
