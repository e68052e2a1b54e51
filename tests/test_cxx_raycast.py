"""GpuLatticeField::raycast (include/field_interpolation/gpu_field.hpp) through libfield_interpolation.so: the C++ program
tests/cxx/test_raycast.cpp casts rays at the mesh of a solved 3-D SDF with both methods and checks the device-pointer and
host-pointer paths of fi_surface_raycast, _count_hits, _contains, _signed_distance and _signed_distance_field against each
other; the results must equal the numpy restatement (tests/ray_reference.py), bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import ray_reference as R
import surface_reference as S
from util import sphere_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_raycast")
SIZES = [40, 36, 32]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_raycast.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_raycast_compiles_and_links():
    if not os.path.exists(os.path.join(PKG, "libfi_hip.so")):
        pytest.skip("libfi_hip.so not built")
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::GpuLatticeField::raycast" in syms


def _read(path):
    out = []
    with open(path, "rb") as f:
        for dtype in (np.float32, np.float32, np.float32, np.float32, np.int64, np.float32, np.int64, np.float32, np.int32,
                      np.uint8, np.uint8, np.float32, np.int64, np.float32, np.float32, np.int64):
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


def _same(got, want):
    assert np.array_equal(np.asarray(got).reshape(-1).view(np.uint32), np.ascontiguousarray(want, np.float32).reshape(-1).view(np.uint32))


@pytest.mark.gpu
def test_cxx_raycast_equals_the_restatement(tmp_path):
    exe = _build()
    pos, nrm = sphere_points(np.random.default_rng(8), SIZES, 2500)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(pos)).tobytes() + pos.tobytes() + nrm.tobytes())
    res = tmp_path / "rays.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all raycast checks passed" in r.stdout
    x, o, d, t0, p0, t1, p1, bary, counts, in_x, in_d, sd, sp, sc, sf, sfp = _read(res)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    for method, t, p in (("iso", t0, p0), ("dual", t1, p1)):
        v, i, _inside = S.surface(x, SIZES, 0.0, method)
        wt, wp, wb, wc = R.cast_and_count(v, i, 3, o, d)
        _same(t, wt)
        assert np.array_equal(p, wp), method
        if method == "iso":
            assert (wp >= 0).sum() > 1000
            _same(bary, wb)
            assert np.array_equal(counts, np.minimum(wc, 2))
            assert np.array_equal(in_x.astype(bool), R.contains(v, i, 3, o))
            assert np.array_equal(in_d.astype(bool), R.contains(v, i, 3, o, [0, -1, 2]))
            wd, wj, wcl = R.signed_distance(v, i, 3, o, 4.0)
            _same(sd, wd)
            assert np.array_equal(sp, wj)
            _same(sc, wcl)
            # the sign pass had something to do: the origins are spread over a 46 x 42 x 38 box and the surface is a sphere
            # of radius 9.3 (util.sphere_points), so 2001 * 3369 / 73416 = 92 of them are expected inside, +- 9.4
            assert np.signbit(wd).sum() > 46
            wf, wfp = R.signed_distance_field(v, i, SIZES)
            _same(sf, wf)
            assert np.array_equal(sfp, wfp)
