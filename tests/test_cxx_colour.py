"""The C++ side of the colour unit through libfield_interpolation.so: the colour members of DepthVolume
(include/field_interpolation/gpu_field.hpp) must give the C ABI's bytes -- the program checks that itself, with host and with
device pointers -- and the Python API's on the same views.  tests/cxx/test_colour.cpp is the program."""
import math
import os
import subprocess

import numpy as np
import pytest

import depth_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_colour")
NEW = ["fi_volume_set_channels", "fi_volume_channels", "fi_volume_colour_load", "fi_volume_colour_copy", "fi_volume_integrate_colour",
       "fi_volume_colour_sample", "fi_volume_render_colour", "fi_volume_colour_constraints"]


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "test_colour.cpp"), "-o", EXE,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cxx_colour_compiles_and_links():
    from field_interpolation_amd import _capi
    assert os.path.exists(os.path.join(PKG, "libfi_hip.so")), "libfi_hip.so is not built"
    assert os.path.exists(_build())
    syms = subprocess.check_output(["nm", "-DC", os.path.join(PKG, "libfield_interpolation.so")], text=True)
    for name in ("set_channels(", "channels(", "integrate_colour(", "copy_colours(", "load_colours(", "sample_colours(", "render_colour(",
                 "colour_constraints("):
        assert "field_interpolation::DepthVolume::" + name in syms, name
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "libfi_hip.so")], text=True).split()
    for name in NEW:
        assert name in exported and name in _capi.SYMBOLS, name


def _read(path, dtypes):
    out = []
    with open(path, "rb") as f:
        for dtype in dtypes:
            n = int(np.frombuffer(f.read(8), np.int64)[0])
            out.append(np.frombuffer(f.read(n * np.dtype(dtype).itemsize), dtype))
    return out


@pytest.mark.gpu
def test_cxx_colour_equals_python(tmp_path):
    import field_interpolation_amd as fi
    exe = _build()
    sizes, centre = [20, 18, 16], np.array([9.5, 8.5, 7.5])
    rng = np.random.default_rng(6)
    cams, depths, colours = [], [], []
    for s in range(ref.CAMERAS + 2):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        h, w = ((17, 33), (24, 24))[s % 2]
        cams.append(ref.look_at(centre + 30.0 * d, centre, np.cross(d, rng.normal(size=3)), math.radians(45.0), w, h, s % 2))
        depths.append((24.0 + rng.uniform(-0.3, 0.3, size=(h, w))).astype(np.float32))   # a blob around the centre
        colours.append(rng.uniform(0.0, 1.0, size=(h, w, 3)).astype(np.float32))
    depths[0][3, 4:9] = (np.nan, np.inf, 0.0, -1.0, np.inf)
    colours[1][2:5, 3:7, 1] = np.nan
    points = (rng.uniform(-0.05, 1.05, size=(2000, 3)) * (np.asarray(sizes) - 1)).astype(np.float32)
    views = tmp_path / "views.bin"
    with open(views, "wb") as f:
        f.write(np.int32(len(cams)).tobytes())
        for c in cams:
            f.write(c.pose.tobytes() + np.array([c.fx, c.fy, c.cx, c.cy], np.float32).tobytes() +
                    np.array([c.width, c.height, c.kind == ref.RANGE], np.int32).tobytes())
        for d in depths:
            f.write(d.tobytes())
        for c in colours:
            f.write(c.tobytes())
        f.write(np.int32(len(points)).tobytes() + points.tobytes())
    res = tmp_path / "colour_out.bin"
    r = subprocess.run([exe, str(views), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all colour checks passed" in r.stdout
    f32, u8 = np.float32, np.uint8
    tsdf, weight, col, cw, sc, sv, depth, image, cp, cc, cwt = _read(res, (f32, f32, f32, f32, f32, u8, f32, f32, f32, f32, f32))
    fc = [fi.Camera(c.pose, c.fx, c.fy, c.cx, c.cy, c.width, c.height, "range" if c.kind == ref.RANGE else "z") for c in cams]
    same = lambda a, b: np.array_equal(np.asarray(a).reshape(-1).view(u8), np.ascontiguousarray(b).reshape(-1).view(u8))  # noqa: E731
    vol = fi.DepthVolume(sizes, 2.5, 4.0, channels=3).integrate(fc, depths, colours=colours)
    assert same(tsdf, vol.tsdf()) and same(weight, vol.weight()) and same(col, vol.colours()) and same(cw, vol.colour_weight())
    want, valid = vol.sample_colours(points, 0.5, valid=True)
    assert same(sc, want) and same(sv, valid) and 0 < valid.sum() < len(valid)
    want = vol.render(fc[-1], colours=True, colour_min_weight=0.5)
    assert same(depth, want[0]) and same(image, want[1]) and np.isfinite(image).any()
    assert all(same(g, w) for g, w in zip((cp, cc, cwt), vol.colour_constraints(1.0)))
