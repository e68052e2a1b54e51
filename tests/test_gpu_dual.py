"""Dual contouring on the device (fi_dual.hip through fi_dual_contour*) against the numpy oracle of the contract
(tests/dual_reference.py) -- vertices, normals, indices and keys bit for bit -- and, in 2-D, against the reference's own
recorded output (tests/golden/dual_contouring_2d_ref.npz)."""
import math

import numpy as np
import pytest

import dual_reference as R
import iso_reference as I
from test_dual_reference import CASES, box, box_gradients, boundary_free, closed_oriented, inside_on_the_left, signed_volume, sphere

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(mesh, ref):
    v, n, idx, keys = ref[:4]
    assert np.array_equal(mesh.keys, keys)
    assert np.array_equal(mesh.indices, idx)
    assert mesh.vertices.shape == v.shape
    assert np.array_equal(bits(mesh.vertices), bits(v))
    assert np.array_equal(bits(mesh.normals), bits(n))


def check(fi, f, sizes, iso=0.0, gradients=None):
    f = np.ascontiguousarray(f, np.float32).reshape(-1)
    mesh = fi.dual_contour(f, sizes, iso, gradients)
    same(mesh, R.contour(f, sizes, iso, gradients))
    return mesh


def smooth(sizes, seed, waves=5, k=0.3):
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sizes[::-1]], indexing="ij")
    f = np.zeros(g[0].shape)
    for _ in range(waves):
        kk = rng.normal(size=len(sizes)) * k
        f += np.cos(sum(a * b for a, b in zip(kk[::-1], g)) + rng.uniform(0, 6.3))
    return f.astype(np.float32).reshape(-1)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_equals_oracle_and_reference(fi, case):
    m = check(fi, case["field"], case["sizes"], case["iso"], case["gradients"])
    assert np.array_equal(bits(m.vertices), bits(case["vertices"]))
    assert np.array_equal(m.indices, case["segments"])


@pytest.mark.parametrize("sizes", [[37, 23], [20, 45], [2, 9], [64, 3], [129, 77]])
def test_non_square_2d(fi, sizes):
    f = smooth(sizes, 4)
    m = check(fi, f, sizes, float(np.median(f)))
    assert len(m.vertices) > 0


def test_caller_gradients_2d_and_3d(fi):
    for sizes, seed in (([33, 21], 5), ([14, 12, 11], 6)):
        f = smooth(sizes, seed)
        g = np.random.default_rng(seed).normal(size=(len(f), len(sizes))).astype(np.float32)
        check(fi, f, sizes, 0.0, g)


@pytest.mark.parametrize("sizes", [[16, 16, 16], [31, 27, 23], [96, 96, 96], [40, 2, 33], [5, 70, 9]])
def test_random_3d(fi, sizes):
    rng = np.random.default_rng(sum(sizes))
    check(fi, rng.normal(size=int(np.prod(sizes))).astype(np.float32), sizes)
    check(fi, smooth(sizes, 2, k=0.4), sizes, -0.2)


def test_spheres_are_closed_with_the_right_volume(fi):
    for sizes, c, r in (([48, 46, 44], (23.3, 22.6, 21.8), 15.3), ([40, 40, 40], (19.5, 19.5, 19.5), 9.0)):
        f = sphere(sizes, c, r)
        m = check(fi, f, sizes)
        assert closed_oriented(m.indices)
        vol = signed_volume(m.vertices, m.indices)
        exact = 4.0 / 3.0 * math.pi * r ** 3
        mc = fi.iso_surface(f, sizes)
        assert abs(vol - exact) <= 0.01 * exact
        assert abs(vol - I.signed_measure(mc.vertices, mc.indices)) <= 0.02 * exact   # (r = 9: 3071.6 against 3031.3)


def test_box_is_closed(fi):
    sizes, c, h = [30, 29, 28], np.array([14.37, 14.21, 13.63]), np.array([8.3, 7.6, 6.15])
    m = check(fi, box(sizes, c, h), sizes)
    assert closed_oriented(m.indices) and signed_volume(m.vertices, m.indices) > 0


def test_2d_inside_on_the_left(fi):
    for case in CASES:
        f = R.distances(case["field"], case["iso"])
        m = fi.dual_contour(case["field"], case["sizes"], case["iso"], case["gradients"])
        assert inside_on_the_left(f, case["sizes"], m.keys, m.indices).all(), case["name"]


# Measured on this field (tests/dual_reference.py gives the same numbers on the CPU): with the analytic gradients every corner
# of the box has a dual-contouring vertex within 1.5e-6 lattice units; fi_iso's nearest vertex is 0.66 .. 1.12 units away.
# Bounds: 0.01 for dual contouring (the issue's), 0.5 below which fi_iso would have to come.
def test_sharp_corners_survive(fi):
    sizes, c, h = [40, 38, 36], np.array([19.37, 18.21, 17.63]), np.array([11.3, 9.6, 8.15])
    f = box(sizes, c, h)
    m = check(fi, f, sizes, 0.0, box_gradients(sizes, c, h))
    corners = np.array([c + h * np.array(s) for s in np.array(np.meshgrid([-1, 1], [-1, 1], [-1, 1])).T.reshape(-1, 3)])

    def nearest(v):
        return np.min(np.linalg.norm(v[None].astype(np.float64) - corners[:, None], axis=2), axis=1)
    dc, mc = nearest(m.vertices), nearest(fi.iso_surface(f, sizes).vertices)
    print("corner distances: dual contouring", dc, "fi_iso", mc)
    assert dc.max() <= 0.01
    assert mc.min() >= 0.5


def test_memory_kinds_and_iso(fi, tmp_path):
    """torch device tensors in (a fresh process, tests/dual_torch_worker.py: torch stays out of this one) give the host
    path's meshes, with and without gradients, through fi.dual_contour and LatticeField.dual_contour"""
    import os
    import subprocess
    import sys
    sizes, iso = [23, 19, 17], 0.4
    f = smooth(sizes, 8)
    g = np.random.default_rng(3).normal(size=(len(f), 3)).astype(np.float32)
    np.savez(tmp_path / "in.npz", sizes=np.array(sizes), f=f, g=g, iso=np.float32(iso))
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dual_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["mixed_refused"][0]
    for name, grads in (("plain", None), ("grad", g), ("ctx", g)):
        host = check(fi, f, sizes, iso, grads)
        for k, v in zip(("vertices", "normals", "indices", "keys"), host):
            assert np.array_equal(o[name + "_" + k], v), (name, k)
    ctx = fi.LatticeField(sizes).dual_contour(f, iso, g)
    for u, w in zip(ctx, check(fi, f, sizes, iso, g)):
        assert np.array_equal(u, w)


def test_two_calls_give_identical_bytes(fi):
    sizes = [50, 44, 41]
    f = smooth(sizes, 11)
    a, b = fi.dual_contour(f, sizes, 0.1), fi.dual_contour(f, sizes, 0.1)
    for u, w in zip(a, b):
        assert u.tobytes() == w.tobytes()


def test_normals_off(fi):
    sizes = [21, 17, 13]
    f = smooth(sizes, 9)
    a, b = fi.dual_contour(f, sizes), fi.dual_contour(f, sizes, normals=False)
    assert b.normals is None and np.array_equal(a.vertices, b.vertices) and np.array_equal(a.indices, b.indices)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_is_invalid(fi, bad):
    for sizes in ([7, 8, 9], [16, 15]):
        f = smooth(sizes, 1)
        f[len(f) // 3] = bad
        with pytest.raises(fi.FiError) as e:
            fi.dual_contour(f, sizes)
        assert e.value.code == 1   # FI_ERR_INVALID


def test_conventions(fi):
    with pytest.raises(fi.FiError) as e:
        fi.dual_contour(np.linspace(-1, 1, 20).astype(np.float32), [20])
    assert e.value.code == 5       # FI_ERR_UNSUPPORTED
    for sizes in ([1, 20, 20], [20, 1], [30, 20, 1]):
        m = fi.dual_contour(smooth(sizes, 2), sizes)
        assert m.vertices.shape == (0, len(sizes)) and m.indices.shape == (0, len(sizes)) and len(m.keys) == 0
    m = fi.dual_contour(np.full(64, 2.0, np.float32), [8, 8])
    assert len(m.vertices) == 0


def test_slab_context_is_unsupported(fi):
    g = fi.LatticeGroup([16, 16, 16], nranks=2)
    r0 = g.members[0]
    with pytest.raises(fi.FiError) as e:
        r0.dual_contour(np.zeros(r0.num_owned, np.float32))
    assert e.value.code == 5


def circle_points(sizes, n):
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    c = (np.array(sizes) - 1) / 2.0
    r = 0.3 * min(sizes)
    return (np.stack([c[0] + r * np.cos(t), c[1] + r * np.sin(t)], 1).astype(np.float32),
            np.stack([np.cos(t), np.sin(t)], 1).astype(np.float32))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_solved_context_in_place(fi, dtype):
    sizes = [60, 50]
    pos, nrm = circle_points(sizes, 400)
    f = fi.sdf_from_points(sizes, fi.Weights(), pos, nrm, dtype=dtype)
    x, it, rel = f.solve_cg(None, 0, 1e-6)
    xs = f.solution_f64().astype(np.float32) if dtype == "f64" else x
    a = f.dual_contour()
    same(a, R.contour(xs, sizes))
    for u, w in zip(a, f.dual_contour(xs)):
        assert np.array_equal(u, w)
    b = f.dual_contour(iso=0.5, gradients=R.calculate_gradients(R.distances(xs, 0.5), sizes))
    same(b, R.contour(xs, sizes, 0.5))


def test_config3_sdf_at_1024(fi):
    from field_interpolation_amd import bench_settings as bs
    from field_interpolation_amd import synth
    sizes, w, pos, nrm = synth.config3(side=1024, points_per_shape=25000, seed=2)
    f = fi.LatticeField(sizes, dtype="f64")
    f.add_field_constraints(w)
    s = bs.SETTINGS[3]   # 4096 -> 1024: two levels less, the same coarsest lattice
    bs.configure(f, s["levels"] - 2, s["coarse_tol"], kcycle=s.get("kcycle", 0), cheb=s.get("cheb"))
    f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
    f.assemble()
    f.solve_cg(None, 0, bs.SETTINGS[3]["tol"])
    xs = f.solution_f64().astype(np.float32)
    m = f.dual_contour()
    same(m, R.contour(xs, sizes))
    assert len(m.vertices) > 1000 and inside_on_the_left(R.distances(xs), sizes, m.keys, m.indices).all()


def test_config5_shape_at_128(fi):
    from field_interpolation_amd import bench_settings as bs
    from field_interpolation_amd import synth
    sizes, w, pos, nrm = synth.config5(side=128, num_points=312500, seed=4)
    f = bs.headline_field(fi, 5, sizes, w, by_field=True)
    f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
    f.assemble()
    f.solve_cg(None, 0, bs.SETTINGS[5]["tol"])
    xs = f.solution_f64().astype(np.float32)
    m = f.dual_contour()
    same(m, R.contour(xs, sizes))
    assert boundary_free(m.indices) and signed_volume(m.vertices, m.indices) > 0
