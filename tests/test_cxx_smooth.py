"""The C++ side of the mesh smoothing through libfield_interpolation.so: GpuLatticeField::iso_surface_smoothed
(include/field_interpolation/gpu_field.hpp) must equal the Python API on the same solved field, and the C ABI walked from C++
with device pointers must agree with it.  tests/cxx/test_smooth.cpp is the program."""
import os
import subprocess

import numpy as np
import pytest

from util import sphere_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_smooth")
SIZES = [40, 36, 32]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_smooth.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_smooth_compiles_and_links():
    if not os.path.exists(os.path.join(PKG, "libfi_hip.so")):
        pytest.skip("libfi_hip.so not built")
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::GpuLatticeField::iso_surface_smoothed" in syms
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "libfi_hip.so")], text=True).split()
    assert "fi_mesh_smooth" in exported and "fi_mesh_normals" in exported


def _read(path, dtypes):
    out = []
    with open(path, "rb") as f:
        for dtype in dtypes:
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_iso_surface_smoothed_equals_python(tmp_path):
    import field_interpolation_amd as fi
    exe = _build()
    pos, nrm = sphere_points(np.random.default_rng(4), SIZES, 2500)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + nrm.tobytes())
    res = tmp_path / "mesh.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all smooth checks passed" in r.stdout
    x, vt, nt, it, vl, nl, il = _read(res, (np.float32, np.float32, np.float32, np.int32, np.float32, np.float32, np.int32))
    laplace = {"iterations": 3, "lam": 0.5, "mu": 0.0, "max_move": 0.25}
    for (v, n, i), mesh in (((vt, nt, it), fi.iso_surface(x, SIZES, smooth=5)),
                            ((vl, nl, il), fi.iso_surface(x, SIZES, largest=1, smooth=laplace))):
        assert len(i) > 0
        assert np.array_equal(v.view(np.uint32), mesh.vertices.reshape(-1).view(np.uint32))
        assert np.array_equal(n.view(np.uint32), mesh.normals.reshape(-1).view(np.uint32))
        assert np.array_equal(i, mesh.indices.reshape(-1))
