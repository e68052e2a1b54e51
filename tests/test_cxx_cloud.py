"""The C++ side of the point-cloud cleaning through libfield_interpolation.so: GpuLatticeField::radius_count,
::neighbour_distances, ::statistical_outliers, ::radius_outliers and the free thin_points
(include/field_interpolation/gpu_field.hpp) must give the C ABI's bytes -- the program checks that itself, with host and with
device pointers -- and the Python API's on the same cloud.  tests/cxx/test_cloud.cpp is the program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cloud_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_cloud")
NEW = ["fi_radius_count", "fi_points_radius_count", "fi_neighbour_distances", "fi_points_neighbour_distances", "fi_outliers_statistical",
       "fi_points_outliers_statistical", "fi_outliers_radius", "fi_points_outliers_radius", "fi_cloud_thin"]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_cloud.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_cloud_compiles_and_links():
    assert os.path.exists(os.path.join(PKG, "libfi_hip.so")), "libfi_hip.so is not built"
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    for name in ("GpuLatticeField::radius_count", "GpuLatticeField::neighbour_distances", "GpuLatticeField::statistical_outliers",
                 "GpuLatticeField::radius_outliers", "thin_points"):
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
def test_cxx_cloud_equals_python(tmp_path):
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    exe = _build()
    pos, _stray = CR.planted_cloud(5, n=1500, planted=15)
    rng = np.random.default_rng(6)
    nrm = rng.normal(size=pos.shape).astype(np.float32)
    q = np.concatenate([pos[:200], rng.uniform(0, 31, size=(200, 3)).astype(np.float32)])
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + nrm.tobytes() + np.int32(len(q)).tobytes() + q.tobytes())
    res = tmp_path / "cloud_out.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all cloud checks passed" in r.stdout
    counts, mean, kth, cnt, stat_keep, radius_keep, raw, tp, tn, tc, ti, cmap = _read(
        res, (np.int32, np.float32, np.float32, np.int32, np.uint8, np.uint8, np.uint8, np.float32, np.float32, np.int32, np.int64,
              np.int32))
    index = fi.PointIndex(pos)
    assert np.array_equal(counts, index.radius_count(q, 1.5, 6))
    m, k, c = index.neighbour_distances(12)
    assert np.array_equal(mean.view(np.uint32), m.view(np.uint32)) and np.array_equal(kth.view(np.uint32), k.view(np.uint32))
    assert np.array_equal(cnt, c)
    keep, stats = index.statistical_outliers(12, 1.0)
    assert np.array_equal(stat_keep.view(np.bool_), keep)
    assert len(raw) == C.sizeof(_capi.FiOutlierStats)
    got = _capi.FiOutlierStats.from_buffer_copy(raw.tobytes())
    assert got.counted == stats["counted"] and got.kept == stats["kept"]
    for key in ("mean", "stddev", "threshold"):
        assert np.float64(getattr(got, key)).tobytes() == np.float64(stats[key]).tobytes(), key
    assert np.array_equal(radius_keep.view(np.bool_), index.radius_outliers(1.5, 2)[0])
    want = fi.thin_points(pos, 0.75, nrm, None, [0.1, 0.2, 0.3], "mean", counts=True, indices=True, cell_map=True)
    for g, w in zip((tp, tn, tc, ti, cmap), want):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).reshape(-1).view(np.uint8))
