"""GpuLatticeField::nearest and ::distance_field (include/field_interpolation/gpu_field.hpp) through
libfield_interpolation.so: the C++ program tests/cxx/test_nearest.cpp queries the points of a 3-D SDF and checks the
device-pointer paths of fi_nearest, fi_distance_field and fi_points_* against the host path; the results must equal the
numpy oracle, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import nearest_reference as R
from util import sphere_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_nearest")
SIZES = [40, 36, 32]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_nearest.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_nearest_compiles_and_links():
    if not os.path.exists(os.path.join(PKG, "libfi_hip.so")):
        pytest.skip("libfi_hip.so not built")
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::GpuLatticeField::nearest" in syms
    assert "field_interpolation::GpuLatticeField::distance_field" in syms


def _read(path):
    out = []
    with open(path, "rb") as f:
        for dtype in (np.float32, np.int64, np.float32, np.int64):
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_nearest_equals_the_oracle(tmp_path):
    exe = _build()
    pos, nrm = sphere_points(np.random.default_rng(7), SIZES, 2500)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + nrm.tobytes())
    res = tmp_path / "nearest.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all nearest checks passed" in r.stdout
    d, i, fd, fi_ = _read(res)
    q = np.concatenate([pos, np.array([[-30, 1, 1], [1, 300, 1], [1, 1, np.nan]], np.float32)])
    wd, wi = R.nearest(pos, q, 3)
    assert np.array_equal(d.view(np.uint32)[:-1], wd.view(np.uint32)[:-1]) and np.isnan(d[-1])
    assert np.array_equal(i, wi)
    assert np.all(d[:len(pos)] == 0)                      # every data point is its own nearest (or ties a duplicate)
    wd, wi = R.distance_field(pos, SIZES)
    assert np.array_equal(fd.view(np.uint32), wd.view(np.uint32))
    assert np.array_equal(fi_, wi)
