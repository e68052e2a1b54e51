"""The C++ side of the mesh parts through libfield_interpolation.so: GpuLatticeField::iso_surface_parts
(include/field_interpolation/gpu_field.hpp) must equal the Python API on the same solved field, and the C ABI walked from
C++ with device pointers must agree with it.  tests/cxx/test_parts.cpp is the program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from util import sphere_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_parts")
SIZES = [40, 36, 32]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_parts.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_parts_compiles_and_links():
    if not os.path.exists(os.path.join(PKG, "libfi_hip.so")):
        pytest.skip("libfi_hip.so not built")
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::GpuLatticeField::iso_surface_parts" in syms


def _read(path, dtypes):
    out = []
    with open(path, "rb") as f:
        for dtype in dtypes:
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_iso_surface_parts_equals_python(tmp_path):
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    exe = _build()
    pos, nrm = sphere_points(np.random.default_rng(4), SIZES, 2500)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + nrm.tobytes())
    res = tmp_path / "mesh.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all parts checks passed" in r.stdout
    x, v, n, i, row = _read(res, (np.float32, np.float32, np.float32, np.int32, np.uint8))
    mesh, parts = fi.iso_surface(x, SIZES, largest=1, parts=True)
    assert np.array_equal(v.view(np.uint32), mesh.vertices.reshape(-1).view(np.uint32))
    assert np.array_equal(n.view(np.uint32), mesh.normals.reshape(-1).view(np.uint32))
    assert np.array_equal(i, mesh.indices.reshape(-1))
    got = _capi.FiMeshPart.from_buffer_copy(row.tobytes())
    assert len(parts.size) == 1 and got.size == parts.size[0] and got.enclosed == parts.enclosed[0]
    assert [getattr(got, k) for k in ("vertices", "primitives", "edges", "boundary", "irregular")] == \
        [int(getattr(parts, k)[0]) for k in ("vertices", "primitives", "edges", "boundary", "irregular")]
    assert list(got.lo) == list(parts.lo[0]) and list(got.hi) == list(parts.hi[0])
    assert C.sizeof(_capi.FiMeshPart) == 80
