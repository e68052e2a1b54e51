"""The C++ side of dual contouring through libfield_interpolation.so: GpuLatticeField::dual_contour
(include/field_interpolation/gpu_field.hpp) must equal the Python API on the same solved field, and the source-compatible
dc::dual_contouring_2d / dc::calculate_gradients (include/field_interpolation/dual_contouring_2d.hpp) must reproduce the
reference's recorded output (tests/golden/dual_contouring_2d_ref.npz).  tests/cxx/test_dual.cpp is the program."""
import os
import subprocess

import numpy as np
import pytest

from test_dual_reference import CASES
from util import sphere_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_dual")
SIZES = [40, 36, 32]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_dual.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_dual_compiles_and_links():
    if not os.path.exists(os.path.join(PKG, "libfi_hip.so")):
        pytest.skip("libfi_hip.so not built")
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    for name in ("field_interpolation::GpuLatticeField::dual_contour", "dc::dual_contouring_2d(", "dc::calculate_gradients("):
        assert name in syms, name


def _read(path, dtypes):
    out = []
    with open(path, "rb") as f:
        for dtype in dtypes:
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_dual_contour_equals_python(tmp_path):
    import field_interpolation_amd as fi
    exe = _build()
    pos, nrm = sphere_points(np.random.default_rng(4), SIZES, 2500)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + nrm.tobytes())
    res = tmp_path / "mesh.bin"
    r = subprocess.run([exe, "solve", str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all dual checks passed" in r.stdout
    x, v, n, i = _read(res, (np.float32, np.float32, np.float32, np.int32))
    py = fi.dual_contour(x, SIZES)
    assert np.array_equal(v.view(np.uint32), py.vertices.reshape(-1).view(np.uint32))
    assert np.array_equal(n.view(np.uint32), py.normals.reshape(-1).view(np.uint32))
    assert np.array_equal(i, py.indices.reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_dropin_reproduces_the_reference(tmp_path, case):
    exe = _build()
    w, h = case["sizes"]
    d = (case["field"].astype(np.float32) - np.float32(case["iso"])).astype(np.float32)
    src = tmp_path / "case.bin"
    with open(src, "wb") as f:
        f.write(np.array([w, h, 0 if case["gradients"] is None else 1], np.int64).tobytes() + d.tobytes())
        if case["gradients"] is not None:
            f.write(np.ascontiguousarray(case["gradients"], np.float32).tobytes())
    res = tmp_path / "out.bin"
    r = subprocess.run([exe, "dc", str(src), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    v, s = _read(res, (np.float32, np.uint32))
    assert np.array_equal(v.view(np.uint32), case["vertices"].reshape(-1).view(np.uint32))
    assert np.array_equal(s.astype(np.int64), case["segments"].reshape(-1).astype(np.int64))
