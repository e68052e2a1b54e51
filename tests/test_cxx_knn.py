"""GpuLatticeField::knn and ::estimate_normals (include/field_interpolation/gpu_field.hpp) through
libfield_interpolation.so: the C++ program tests/cxx/test_knn.cpp queries the points of a 3-D SDF and checks the
device-pointer paths of fi_knn, fi_estimate_normals and fi_points_* against the host path; the results must equal the
numpy oracle, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import normals_reference as R
from util import sphere_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_knn")
SIZES = [40, 36, 32]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_knn.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_knn_compiles_and_links():
    assert os.path.exists(os.path.join(PKG, "libfi_hip.so")), "libfi_hip.so not built"
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::GpuLatticeField::knn" in syms
    assert "field_interpolation::GpuLatticeField::estimate_normals" in syms


def _read(path):
    out = []
    with open(path, "rb") as f:
        for dtype in (np.float32, np.int64, np.float32, np.float32):
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_knn_equals_the_oracle(tmp_path):
    exe = _build()
    pos, _ = sphere_points(np.random.default_rng(7), SIZES, 2500)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes())
    res = tmp_path / "knn.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all knn checks passed" in r.stdout
    d, i, nrm, var = _read(res)
    q = np.concatenate([pos, np.array([[-30, 1, 1], [1, 1, np.nan]], np.float32)])
    wd, wi = R.knn(pos, q, 3, 10)
    d, i = d.reshape(-1, 10), i.reshape(-1, 10)
    assert np.array_equal(d.view(np.uint32)[:-1], wd.view(np.uint32)[:-1]) and np.all(np.isnan(d[-1]))
    assert np.array_equal(i, wi)
    assert np.all(d[:len(pos), 0] == 0)                   # every data point is its own nearest (or ties a duplicate)
    wn, wv = R.estimate_normals(pos, 3, 12, viewpoints=np.array([[-40.0, 17.5, 15.5]], np.float32))
    assert np.array_equal(nrm.reshape(-1, 3).view(np.uint32), wn.view(np.uint32))
    assert np.array_equal(var.view(np.uint32), wv.view(np.uint32))
