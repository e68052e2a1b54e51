"""The C++ side of the march unit through libfield_interpolation.so: DepthVolume::raycast / render and
GpuLatticeField::march / render (include/field_interpolation/gpu_field.hpp) must give the C ABI's bytes -- the program checks
that itself, with host and with device pointers -- and the Python API's and the definition's on the same case.
tests/cxx/test_march.cpp is the program."""
import os
import subprocess

import numpy as np
import pytest

import march_cases as cases
import march_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_march")
NEW = ["fi_march_default_options", "fi_field_raycast", "fi_field_render", "fi_raycast_field", "fi_render_field", "fi_volume_raycast",
       "fi_volume_render"]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_march.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_march_compiles_and_links():
    assert os.path.exists(os.path.join(PKG, "libfi_hip.so")), "libfi_hip.so is not built"
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    for name in ("DepthVolume::raycast(", "DepthVolume::render(", "GpuLatticeField::march(", "GpuLatticeField::render("):
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
def test_cxx_march_equals_python_and_the_definition(tmp_path):
    import field_interpolation_amd as fi
    exe = _build()
    t, W = cases.fused(cases.SPHERE)
    cam = cases.sphere_camera(33)
    rng = np.random.default_rng(17)
    hi = np.array(cases.SIZES, np.float64) - 1
    o = (rng.uniform(-0.3, 1.3, size=(600, 3)) * hi).astype(np.float32)
    d = (rng.uniform(0.2, 0.8, size=(600, 3)) * hi - o).astype(np.float32)
    case = tmp_path / "case.bin"
    with open(case, "wb") as f:
        f.write(np.array(cases.SIZES, np.int32).tobytes() + t.tobytes() + W.tobytes())
        f.write(cam.pose.tobytes() + np.array([cam.fx, cam.fy, cam.cx, cam.cy], np.float32).tobytes() +
                np.array([cam.width, cam.height, 1], np.int32).tobytes())
        f.write(np.int32(len(o)).tobytes() + o.tobytes() + d.tobytes())
    res = tmp_path / "march_out.bin"
    r = subprocess.run([exe, str(case), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all march checks passed" in r.stdout
    f32 = np.float32
    got = _read(res, (f32, f32, f32, np.int8, f32, f32, f32, f32))
    same = lambda a, b: np.array_equal(np.asarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))  # noqa: E731
    vol = fi.DepthVolume(cases.SIZES, 3.0).load(t, W)
    rays = vol.raycast(o, d, step=0.7, side="either", positions=True, normals=True)        # (t, side, positions, normals)
    assert all(same(g, w) for g, w in zip((got[0], got[3], got[1], got[2]), rays))
    want = ref.raycast(t, cases.SIZES, o, d, step=0.7, side=ref.EITHER, weight=W)
    assert all(same(g, w) for g, w in zip(got[:4], want))
    fcam = fi.Camera(cam.pose, cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, "range")
    # (the program renders with its ray options: step 0.7, either side)
    want = ref.render(t, cases.SIZES, cam, step=0.7, side=ref.EITHER, weight=W)
    assert all(same(g, w) for g, w in zip(got[4:], want))
    image = vol.render(fcam, step=0.7, positions=True, normals=True, incidence=True)       # front crossings only
    front = ref.render(t, cases.SIZES, cam, step=0.7, weight=W)
    assert all(same(g, w) for g, w in zip(image, front))
