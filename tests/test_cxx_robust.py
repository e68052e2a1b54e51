"""GpuLatticeField::solve_robust and ::point_residuals (include/field_interpolation/gpu_field.hpp) through
libfield_interpolation.so: the C++ program tests/cxx/test_robust.cpp fits the 2-D value data with gross errors of
tests/robust_reference.py in fp32.  The residuals must equal the numpy restatement bit for bit; the robust field may be 4x
as far from the fp64 reference loop as the plain fp32 solve is from the oracle's exact solve (tests/test_gpu_robust.py)."""
import os
import subprocess

import numpy as np
import pytest

import robust_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_robust")
SIZES = [64, 64]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_robust.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_robust_compiles_and_links():
    if not os.path.exists(os.path.join(PKG, "libfi_hip.so")):
        pytest.skip("libfi_hip.so not built")
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    assert "field_interpolation::GpuLatticeField::solve_robust" in syms
    assert "field_interpolation::GpuLatticeField::point_residuals" in syms


def _read(path):
    out = []
    with open(path, "rb") as f:
        for _ in range(4):
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * 4), np.float32))
        out += list(np.frombuffer(f.read(16), np.int64))
    return out


@pytest.mark.gpu
def test_cxx_robust_equals_the_references(tmp_path):
    from oracle import fi_oracle
    exe = _build()
    b, bad = R.noisy_value_data(SIZES, 3000, 1)
    pts = tmp_path / "points.bin"
    with open(pts, "wb") as f:
        f.write(np.int32(len(b["pos"])).tobytes() + b["pos"].tobytes() + b["val"].tobytes())
    res = tmp_path / "robust.bin"
    r = subprocess.run([exe, str(pts), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all robust checks passed" in r.stdout
    plain, resid, robust, omega, it_plain, it_all = _read(res)
    # every point was added on its own: 3000 batches of one point, numbered in call order
    want = R.residuals(SIZES, [b], plain, np.float32)
    assert np.array_equal(resid.view(np.uint32), want.view(np.uint32))
    x, om, fields = R.irls(SIZES, fi_oracle.Weights(model_2=3.0), [b], loss=R.HUBER, rounds=5)
    dist = lambda a, ref: float(np.abs(a.astype(np.float64) - ref).max() / np.abs(ref).max())  # noqa: E731
    d0, d = dist(plain, fields[0]), dist(robust, x)
    assert d <= 4 * d0, "plain fp32 solve to the exact solve: %.3g; robust field to the reference loop: %.3g" % (d0, d)
    truth = R.truth_on_lattice(SIZES)
    assert R.rms(robust, truth) <= 0.25 * R.rms(plain, truth)
    assert omega[bad].mean() < 0.2 < 0.8 < omega[~bad].mean()
    assert it_all > it_plain > 0
