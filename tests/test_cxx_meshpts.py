"""The C++ side of the mesh sampling through libfield_interpolation.so: GpuLatticeField::iso_surface_points
(include/field_interpolation/gpu_field.hpp) must equal sample_mesh(iso_surface(...), normals="vertex") of the Python API on the
same solved field, and the C ABI walked from C++ with device pointers must agree with it.  tests/cxx/test_meshpts.cpp is the
program."""
import os
import subprocess

import numpy as np
import pytest

from util import sphere_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_meshpts")
SIZES = [40, 36, 32]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_meshpts.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_meshpts_compiles_and_links():
    if not os.path.exists(os.path.join(PKG, "libfi_hip.so")):
        pytest.skip("libfi_hip.so not built")
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::GpuLatticeField::iso_surface_points" in syms
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "libfi_hip.so")], text=True).split()
    assert "fi_mesh_sample" in exported and "fi_mesh_deviation" in exported


def _read(path, dtypes):
    out = []
    with open(path, "rb") as f:
        for dtype in dtypes:
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_iso_surface_points_equals_python(tmp_path):
    import field_interpolation_amd as fi
    exe = _build()
    pos, nrm = sphere_points(np.random.default_rng(4), SIZES, 2500)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + nrm.tobytes())
    res = tmp_path / "points_out.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all meshpts checks passed" in r.stdout
    x, pi, ni, pd, nd = _read(res, (np.float32,) * 5)
    for (p, n), mesh in (((pi, ni), fi.iso_surface(x, SIZES)), ((pd, nd), fi.dual_contour(x, SIZES))):
        want_p, want_n = fi.sample_mesh(mesh, 5000, 9, normals="vertex")
        assert np.array_equal(p.view(np.uint32), want_p.reshape(-1).view(np.uint32))
        assert np.array_equal(n.view(np.uint32), want_n.reshape(-1).view(np.uint32))
