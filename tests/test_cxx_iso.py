"""GpuLatticeField::iso_surface (include/field_interpolation/gpu_field.hpp) through libfield_interpolation.so: the C++
program tests/cxx/test_iso.cpp solves a 3-D SDF, extracts its iso-surface from the solution on the device and checks the
device-resident paths of the C ABI against it; the mesh must equal the Python API's on the same solved field."""
import os
import subprocess

import numpy as np
import pytest

from util import sphere_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_iso")
SIZES = [40, 36, 32]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_iso.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_iso_compiles_and_links():
    if not os.path.exists(os.path.join(PKG, "libfi_hip.so")):
        pytest.skip("libfi_hip.so not built")
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::GpuLatticeField::iso_surface" in syms


def _read(path):
    out = []
    with open(path, "rb") as f:
        for dtype in (np.float32, np.float32, np.float32, np.int32):
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_iso_surface_equals_python(tmp_path):
    import field_interpolation_amd as fi
    exe = _build()
    pos, nrm = sphere_points(np.random.default_rng(4), SIZES, 2500)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + nrm.tobytes())
    res = tmp_path / "mesh.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all iso checks passed" in r.stdout
    x, v, n, i = _read(res)
    py = fi.iso_surface(x, SIZES)
    assert np.array_equal(v.view(np.uint32), py.vertices.reshape(-1).view(np.uint32))
    assert np.array_equal(n.view(np.uint32), py.normals.reshape(-1).view(np.uint32))
    assert np.array_equal(i, py.indices.reshape(-1))
    # the same problem solved from Python gives the same field, so the same surface up to the solver's tolerance
    f = fi.sdf_from_points(SIZES, fi.Weights(), pos, nrm)
    f.set_levels(3)
    f.set_multigrid(True)
    xp, it, rel = f.solve_cg(None, 0, 1e-6)
    assert np.abs(xp - x).max() <= 1e-3 * np.abs(x).max()
    mp = f.iso_surface()
    assert abs(len(mp.vertices) - len(v) // 3) <= 0.01 * len(v) // 3
