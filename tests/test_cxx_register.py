"""The C++ side of the registration through libfield_interpolation.so: GpuLatticeField::register_points
(include/field_interpolation/gpu_field.hpp) must equal register_points(cloud, iso_surface(...)) of the Python API on the same
solved field in every byte of the result, and the C ABI walked from C++ with device pointers must agree with it.
tests/cxx/test_register.cpp is the program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import register_reference as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_register")
SIZES = [40, 36, 32]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_register.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_register_compiles_and_links():
    assert os.path.exists(os.path.join(PKG, "libfi_hip.so")), "libfi_hip.so is not built"
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::GpuLatticeField::register_points" in syms
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "libfi_hip.so")], text=True).split()
    assert "fi_mesh_register" in exported and "fi_points_register" in exported


def _read(path, dtypes):
    out = []
    with open(path, "rb") as f:
        for dtype in dtypes:
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


def ellipsoid_points(rng, n):
    """n oriented points of an ellipsoid of half-axes (12, 10, 8) in the middle of the lattice, and 700 of them turned and shifted"""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axes = np.array([12.0, 10.0, 8.0])
    pos = ((np.array(SIZES) - 1) / 2.0 + d * axes).astype(np.float32)
    nrm = d / axes
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    return pos, nrm, G.moved(pos[:700], G.rotation((2, -1, 3), 5.0), (0.4, -0.3, 0.35))


@pytest.mark.gpu
def test_cxx_register_points_equals_python(tmp_path):
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    exe = _build()
    pos, nrm, cloud = ellipsoid_points(np.random.default_rng(4), 2500)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + nrm.tobytes() + np.int32(len(cloud)).tobytes() + cloud.tobytes())
    res = tmp_path / "register_out.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all register checks passed" in r.stdout
    x, si, sd, moved, dist, _sp = _read(res, (np.float32, np.uint8, np.uint8, np.float32, np.float32, np.uint8))
    assert len(si) == len(sd) == C.sizeof(_capi.FiRegistration)
    for raw, mesh in ((si, fi.iso_surface(x, SIZES)), (sd, fi.dual_contour(x, SIZES))):
        got = _capi.FiRegistration.from_buffer_copy(raw.tobytes())
        want = fi.register_points(cloud, mesh, max_iterations=6, transformed=True, distances=True)
        assert np.array_equal(np.array(list(got.transform)).view(np.uint64)[:16].reshape(4, 4), want["transform"].view(np.uint64))
        for k in ("iterations", "converged", "fixed_mask", "queries", "counted", "beyond", "invalid", "degenerate"):
            assert getattr(got, k) == want[k], k
        for k in ("rms", "weighted_rms", "last_rotation", "last_translation"):
            assert np.float64(getattr(got, k)).tobytes() == np.float64(want[k]).tobytes(), k
        assert want["counted"] == len(cloud) and 0 < want["iterations"] <= 6
        if raw is si:
            assert np.array_equal(moved.view(np.uint32), want["transformed"].reshape(-1).view(np.uint32))
            assert np.array_equal(dist.view(np.uint32), want["distances"].view(np.uint32))
