"""Iso-contours and iso-surfaces on the device (fi_iso.hip through fi_iso_extract*) against the numpy oracle of the
contract (tests/iso_reference.py): keys and indices equal, positions bit-equal, normals within 1e-5."""
import math

import numpy as np
import pytest

import iso_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _same(mesh, ref):
    v, n, idx, keys = ref
    assert np.array_equal(mesh.keys, keys)
    assert np.array_equal(mesh.indices, idx)
    assert mesh.vertices.shape == v.shape
    assert np.array_equal(mesh.vertices.view(np.uint32), v.view(np.uint32))
    if len(n):
        assert np.abs(mesh.normals - n).max() <= 1e-5


def _check(fi, f, sizes, iso=0.0):
    f = np.ascontiguousarray(f, np.float32).reshape(-1)
    mesh = fi.iso_surface(f, sizes, iso)
    _same(mesh, R.extract(f, sizes, iso))
    return mesh


def _sphere(sizes, c, r):
    g = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sizes[::-1]], indexing="ij")
    d2 = sum((g[len(sizes) - 1 - k] - c[k]) ** 2 for k in range(len(sizes)))
    return (np.sqrt(d2) - r).astype(np.float32).reshape(-1)


def _smooth(sizes, seed):
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sizes[::-1]], indexing="ij")
    f = np.zeros(g[0].shape)
    for _ in range(5):
        k = rng.normal(size=len(sizes)) * 0.3
        f += np.cos(sum(kk * gg for kk, gg in zip(k[::-1], g)) + rng.uniform(0, 6.3))
    return f.astype(np.float32).reshape(-1)


@pytest.mark.parametrize("case", range(16))
def test_every_square_case(fi, case):
    f = np.array([-1.0 if (case >> k) & 1 else 1.0 for k in range(4)], np.float32) * np.array([0.3, 0.7, 1.1, 0.5], np.float32)
    m = _check(fi, f, [2, 2])
    assert len(m.indices) == len(R.cell_primitives(2, R.case_inside(2, case)))


@pytest.mark.parametrize("case", range(256))
def test_every_cube_case(fi, case):
    mags = np.array([0.3, 0.7, 1.1, 0.5, 0.9, 0.2, 0.6, 1.3], np.float32)
    f = np.array([-1.0 if (case >> k) & 1 else 1.0 for k in range(8)], np.float32) * mags
    m = _check(fi, f, [2, 2, 2])
    assert len(m.indices) == len(R.cell_primitives(3, R.case_inside(3, case)))


@pytest.mark.parametrize("sizes", [[9, 8, 7], [12, 11]])
def test_checkerboard(fi, sizes):
    g = np.indices(sizes[::-1]).sum(axis=0)
    f = np.where(g % 2 == 0, -1.0, 1.0).astype(np.float32) * (1 + 0.1 * (np.arange(g.size) % 7).reshape(g.shape))
    m = _check(fi, f, sizes)
    assert len(m.indices) > 0


@pytest.mark.parametrize("sizes", [[67, 33, 19], [1, 20, 20], [20, 1, 20], [2, 2, 2], [1024, 1024], [1, 50], [33, 2, 5]])
def test_sizes(fi, sizes):
    _check(fi, _smooth(sizes, 3), sizes, 0.2)


def test_values_equal_to_iso(fi):
    sizes = [13, 11, 9]
    f = np.round(_smooth(sizes, 5) * 2) / 2  # many values exactly 0.5, 0, -0.5
    _check(fi, f, sizes, 0.5)
    _check(fi, f, sizes, 0.0)
    _check(fi, f[:13 * 11], [13, 11], 0.5)


def test_constant_field_is_empty(fi):
    for sizes in ([8, 9, 10], [30, 40]):
        m = fi.iso_surface(np.full(int(np.prod(sizes)), 2.0, np.float32), sizes)
        assert m.vertices.shape == (0, len(sizes)) and m.indices.shape == (0, len(sizes)) and len(m.keys) == 0


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_is_invalid(fi, bad):
    for sizes in ([7, 8, 9], [16, 15]):
        f = _smooth(sizes, 1)
        f[len(f) // 3] = bad
        with pytest.raises(fi.FiError) as e:
            fi.iso_surface(f, sizes)
        assert e.value.code == 1   # FI_ERR_INVALID


def test_one_dimensional_is_unsupported(fi):
    with pytest.raises(fi.FiError) as e:
        fi.iso_surface(np.linspace(-1, 1, 20).astype(np.float32), [20])
    assert e.value.code == 5       # FI_ERR_UNSUPPORTED


def test_analytic_sphere(fi):
    sizes, c, r = [96, 96, 96], (47.3, 48.1, 46.7), 30.3
    f = _sphere(sizes, c, r)
    m = _check(fi, f, sizes)
    assert len(m.vertices) == 17298
    rad = np.linalg.norm(m.vertices.astype(np.float64) - np.array(c), axis=1)
    assert np.abs(rad - r).max() < 0.01
    assert R.watertight_oriented(m.indices)
    assert R.euler_characteristic(len(m.vertices), m.indices) == 2
    vol = R.signed_measure(m.vertices, m.indices)
    assert abs(vol - 4 / 3 * math.pi * r ** 3) < 0.01 * 4 / 3 * math.pi * r ** 3


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_solution_none_equals_out(fi, dtype):
    sizes = [24, 22, 20]
    rng = np.random.default_rng(1)
    d = rng.normal(size=(1500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = ((np.array(sizes) - 1) / 2.0 + 7.0 * d).astype(np.float32)
    f = fi.sdf_from_points(sizes, fi.Weights(), pos, d.astype(np.float32), dtype=dtype)
    x, it, rel = f.solve_cg(None, 0, 1e-6)
    a = f.iso_surface()
    b = f.iso_surface(x)
    _same(a, R.extract(x, sizes))
    for u, w in zip(a, b):
        assert np.array_equal(u, w)
    c = fi.iso_surface(x, sizes)
    for u, w in zip(a, c):
        assert np.array_equal(u, w)


def test_2d_context_solution(fi):
    sizes = [60, 50]
    t = np.linspace(0, 2 * np.pi, 400, endpoint=False)
    pos = np.stack([29.5 + 15 * np.cos(t), 24.5 + 15 * np.sin(t)], 1).astype(np.float32)
    nrm = np.stack([np.cos(t), np.sin(t)], 1).astype(np.float32)
    f = fi.sdf_from_points(sizes, fi.Weights(), pos, nrm)
    x, it, rel = f.solve_cg(None, 0, 1e-6)
    m = f.iso_surface()
    _same(m, R.extract(x, sizes))
    assert R.watertight_oriented(m.indices)
    assert abs(R.signed_measure(m.vertices, m.indices) - math.pi * 15 ** 2) < 0.05 * math.pi * 15 ** 2


def test_sdf_sphere_end_to_end(fi):
    sizes, c, r = [64, 64, 64], np.array([31.5, 31.5, 31.5]), 20.0
    rng = np.random.default_rng(2)
    d = rng.normal(size=(20000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = (c + r * d).astype(np.float32)
    f = fi.sdf_from_points(sizes, fi.Weights(), pos, d.astype(np.float32))
    f.set_levels(4)
    f.set_multigrid(True)
    x, it, rel = f.solve_cg(None, 0, 1e-5)
    m = f.iso_surface()
    _same(m, R.extract(x, sizes))
    assert R.watertight_oriented(m.indices)
    assert R.components(len(m.vertices), m.indices) == 1
    assert R.euler_characteristic(len(m.vertices), m.indices) == 2
    vol = R.signed_measure(m.vertices, m.indices)
    assert abs(vol - 4 / 3 * math.pi * r ** 3) < 0.05 * 4 / 3 * math.pi * r ** 3, vol


def test_normals_off_and_device_free_call_agree(fi):
    sizes = [21, 17, 13]
    f = _smooth(sizes, 9)
    a = fi.iso_surface(f, sizes, 0.1)
    b = fi.iso_surface(f, sizes, 0.1, normals=False)
    assert b.normals is None and np.array_equal(a.vertices, b.vertices) and np.array_equal(a.indices, b.indices)
