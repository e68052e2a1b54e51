"""GpuLatticeField::redistance (include/field_interpolation/gpu_field.hpp) through libfield_interpolation.so: the C++ program
tests/cxx/test_surface.cpp redistances a solved 3-D SDF with both methods and checks the device-pointer paths of
fi_redistance_field and fi_surface_* (from a mesh, from host arrays, from device arrays) against each other; the results
must equal the numpy oracle, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import surface_reference as S
from util import sphere_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_surface")
SIZES = [40, 36, 32]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_surface.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_surface_compiles_and_links():
    if not os.path.exists(os.path.join(PKG, "libfi_hip.so")):
        pytest.skip("libfi_hip.so not built")
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::GpuLatticeField::redistance" in syms


def _read(path):
    out = []
    with open(path, "rb") as f:
        for dtype in (np.float32, np.float32, np.int64, np.float32, np.int64, np.float32, np.int32, np.float32, np.float32,
                      np.int64, np.float32):
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_surface_equals_the_oracle(tmp_path):
    exe = _build()
    pos, nrm = sphere_points(np.random.default_rng(8), SIZES, 2500)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + nrm.tobytes())
    res = tmp_path / "surface.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all surface checks passed" in r.stdout
    x, d0, p0, d1, p1, v, idx, q, qd, qp, qc = _read(res)
    for method, d, p in (("iso", d0, p0), ("dual", d1, p1)):
        wd, wp = S.redistance(x, SIZES, 0.0, method)
        assert np.array_equal(d.view(np.uint32), wd.view(np.uint32)), method
        assert np.array_equal(p, wp), method
    wv, wi, _inside = S.surface(x, SIZES, 0.0, "iso")
    assert np.array_equal(v.view(np.uint32), wv.reshape(-1).view(np.uint32)) and np.array_equal(idx, wi.reshape(-1))
    wd, wp, wc = S.distance(wv, wi, q, 3)
    assert np.array_equal(qd.view(np.uint32), wd.view(np.uint32))
    assert np.array_equal(qp, wp)
    assert np.array_equal(qc.view(np.uint32), wc.reshape(-1).view(np.uint32))
