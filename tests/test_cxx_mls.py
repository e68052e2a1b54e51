"""The C++ side of the moving-least-squares projection through libfield_interpolation.so: GpuLatticeField::smooth_points and
the free smooth_points (include/field_interpolation/gpu_field.hpp) must give the C ABI's bytes -- the program checks that
itself, with host and with device pointers -- and the Python API's on the same cloud.  tests/cxx/test_mls.cpp is the
program."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_mls")
NEW = ["fi_mls_project", "fi_points_mls_project"]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_mls.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_mls_compiles_and_links():
    assert os.path.exists(os.path.join(PKG, "libfi_hip.so")), "libfi_hip.so is not built"
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    for name in ("GpuLatticeField::smooth_points(", "smooth_points(int"):
        assert "field_interpolation::" + name in syms, name
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "libfi_hip.so")], text=True).split()
    for name in NEW:
        assert name in exported, name


def _read(path, dtypes):
    out = []
    with open(path, "rb") as f:
        for dtype in dtypes:
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_mls_equals_python(tmp_path):
    import field_interpolation_amd as fi
    exe = _build()
    rng = np.random.default_rng(5)
    d = rng.normal(size=(1500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = (15.5 + 9.0 * d + rng.normal(scale=0.05, size=d.shape)).astype(np.float32)     # a noisy sphere in a 32^3 lattice
    guide = d.astype(np.float32)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + guide.tobytes())
    res = tmp_path / "mls_out.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all mls checks passed" in r.stdout
    p, nr, cu, od, q, qo = _read(res, (np.float32, np.float32, np.float32, np.uint8, np.float32, np.uint8))
    index = fi.PointIndex(pos)
    want = index.smooth(k=32, radius=2.5, degree=2, max_move=0.5, normals=guide, curvature=True, order=True)
    for g, w in zip((p, nr, cu, od), want):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).reshape(-1).view(np.uint8))
    assert np.all((nr.reshape(-1, 3) * guide).sum(1)[od > 0] > 0)            # the guides' orientation: outward
    plane = index.smooth(k=32, radius=2.5, degree=1, order=True)
    assert np.array_equal(q.view(np.uint32), plane[0].reshape(-1).view(np.uint32)) and np.array_equal(qo, plane[2])
    also = fi.smooth_points(pos, 2.5, max_move=0.5, normals=guide, curvature=True, order=True)
    assert all(np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)) for a, b in zip(also, want))
