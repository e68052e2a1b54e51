"""The C++ side of the clustering through libfield_interpolation.so: GpuLatticeField::cluster_points
(include/field_interpolation/gpu_field.hpp) must give the C ABI's bytes -- the program checks that itself, with host and with
device pointers, and takes fi_cluster_measure's table both ways -- and the Python API's on the same cloud.
tests/cxx/test_cluster.cpp is the program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cluster_reference as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_cluster")
NEW = ["fi_cluster", "fi_points_cluster", "fi_cluster_measure"]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_cluster.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_cluster_compiles_and_links():
    assert os.path.exists(os.path.join(PKG, "libfi_hip.so")), "libfi_hip.so is not built"
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::GpuLatticeField::cluster_points" in syms
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "libfi_hip.so")], text=True).split()
    for name in NEW:
        assert name in exported, name


def test_struct_mirrors_match_the_header():
    from field_interpolation_amd import _capi
    assert C.sizeof(_capi.FiClusterStats) == 5 * C.sizeof(C.c_long)
    assert C.sizeof(_capi.FiClusterRow) == 2 * C.sizeof(C.c_long) + 6 * 4 + 3 * 8
    assert [f for f, _ in _capi.FiClusterStats._fields_] == ["clusters", "core", "border", "noise", "non_finite"]
    assert [f for f, _ in _capi.FiClusterRow._fields_] == ["count", "core", "lo", "hi", "centroid"]


def _read(path, dtypes):
    out = []
    with open(path, "rb") as f:
        for dtype in dtypes:
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_cluster_equals_python(tmp_path):
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    exe = _build()
    pos, _clump = KR.clump_cloud(5)
    nrm = np.random.default_rng(6).normal(size=pos.shape).astype(np.float32)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + nrm.tobytes())
    res = tmp_path / "cluster_out.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all cluster checks passed" in r.stdout
    labels1, core1, labels4, core4, raw1, raw4, rows = _read(res, (np.int32, np.uint8, np.int32, np.uint8, np.uint8, np.uint8, np.uint8))
    index = fi.PointIndex(pos)
    for (eps, least), labels, core, raw in (((1.5, 1), labels1, core1, raw1), ((0.6, 4), labels4, core4, raw4)):
        want_labels, want_core, stats = index.cluster(eps, least, core=True, stats=True)
        assert np.array_equal(labels, want_labels) and np.array_equal(core.view(np.bool_), want_core)
        assert len(raw) == C.sizeof(_capi.FiClusterStats)
        got = _capi.FiClusterStats.from_buffer_copy(raw.tobytes())
        assert {k: getattr(got, k) for k in stats} == stats
    table = fi.cluster_measure(pos, labels1, core1)
    assert len(rows) == len(table) * C.sizeof(_capi.FiClusterRow)
    for c, want in enumerate(table):
        got = _capi.FiClusterRow.from_buffer_copy(rows.tobytes(), c * C.sizeof(_capi.FiClusterRow))
        assert got.count == want["count"] and got.core == want["core"]
        assert np.float32(got.lo[:]).tobytes() == want["lo"].tobytes() and np.float32(got.hi[:]).tobytes() == want["hi"].tobytes()
        assert np.float64(got.centroid[:]).tobytes() == want["centroid"].tobytes()
