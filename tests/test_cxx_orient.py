"""GpuLatticeField::orient_normals (include/field_interpolation/gpu_field.hpp) through libfield_interpolation.so: the C++
program tests/cxx/test_orient.cpp orients normals at the points of a 3-D SDF and checks the device-pointer paths of
fi_orient_normals and fi_points_orient_normals against the host path; the results must equal the numpy restatement
(tests/orient_reference.py), bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import orient_reference as O
from util import sphere_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_orient")
SIZES = [40, 36, 32]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_orient.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_orient_compiles_and_links():
    assert os.path.exists(os.path.join(PKG, "libfi_hip.so")), "libfi_hip.so not built"
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::GpuLatticeField::orient_normals" in syms


def _read(path):
    out = []
    with open(path, "rb") as f:
        for dtype in (np.float32, np.int64, np.float32, np.int64):
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_orient_equals_the_restatement(tmp_path):
    exe = _build()
    rng = np.random.default_rng(7)
    pos, _ = sphere_points(rng, SIZES, 2500)
    nrm = rng.normal(size=pos.shape).astype(np.float32)
    nrm[::60] = 0.0                                        # dead points
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + nrm.tobytes())
    res = tmp_path / "orient.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all orient checks passed" in r.stdout
    n0, c0, n1, c1 = _read(res)
    for got_n, got_c, kw in ((n0, c0, {}), (n1, c1, {"viewpoints": np.array([[-400.0, 17.5, 15.5]], np.float32)})):
        wn, wc = O.orient_normals(pos, nrm, 3, 10, **kw)
        assert np.array_equal(got_n.reshape(-1, 3).view(np.uint32), wn.view(np.uint32))
        assert np.array_equal(got_c, wc)
