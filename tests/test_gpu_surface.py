"""Distances to a surface and redistancing on the device (fi_surface.hip through fi_surface_* / fi_redistance*) against the
numpy oracle of the contract (tests/surface_reference.py) -- distances as bits, primitive indices, closest points and signs
bit for bit -- and an analytic sphere's signed distance."""
import ctypes as C
import math

import numpy as np
import pytest

import surface_reference as S
from nearest_reference import lattice_points

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(got, want):
    assert got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)), np.flatnonzero(bits(got) != bits(want))[:10]


def smooth(sizes, seed, waves=5, k=0.3):
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sizes[::-1]], indexing="ij")
    f = np.zeros(g[0].shape)
    for _ in range(waves):
        kk = rng.normal(size=len(sizes)) * k
        f += np.cos(sum(a * b for a, b in zip(kk[::-1], g)) + rng.uniform(0, 6.3))
    return f.astype(F).reshape(-1)


def check_lattice(fi, f, sizes, iso, method, max_distance=math.inf):
    """the whole lattice: module-level redistance, a context's redistance with primitives and its mesh, and the unsigned
    distance field of that mesh"""
    want, wj = S.redistance(f, sizes, iso, method, max_distance)
    same_bits(fi.redistance(f, sizes, iso, method, max_distance), want)
    ctx = fi.LatticeField(sizes)
    d, j, mesh = ctx.redistance(f, iso, method, max_distance, primitives=True)
    same_bits(d, want)
    assert np.array_equal(j, wj)
    v, i, _inside = S.surface(f, sizes, iso, method)
    assert np.array_equal(bits(mesh.vertices), bits(v)) and np.array_equal(mesh.indices, i)
    if len(i):
        u, uj = fi.SurfaceIndex.from_mesh(mesh).distance_field(sizes, max_distance, primitives=True)
        same_bits(u, np.abs(want))
        assert np.array_equal(uj, wj)
    return want, wj, mesh


@pytest.mark.parametrize("method", ["iso", "dual"])
@pytest.mark.parametrize("sizes", [[2, 2], [2, 9], [31, 17], [128, 128], [2, 2, 2], [7, 5, 6], [24, 24, 24], [2, 13, 11]])
def test_full_lattices(fi, sizes, method):
    f = smooth(sizes, sum(sizes))
    check_lattice(fi, f, sizes, float(np.median(f)), method)


@pytest.mark.parametrize("method", ["iso", "dual"])
def test_max_distance(fi, method):
    sizes = [20, 18, 16]
    f = smooth(sizes, 7)
    for md in (0.0, 0.5, 2.0, math.inf):
        d, _j, _m = check_lattice(fi, f, sizes, 0.1, method, md)
        assert np.all(np.isinf(d) == (np.abs(d) > md))


@pytest.mark.parametrize("method", ["iso", "dual"])
def test_integer_fields_give_degenerate_triangles(fi, method):
    rng = np.random.default_rng(11)
    for sizes in ([13, 11, 9], [30, 27]):
        f = rng.integers(-2, 3, size=int(np.prod(sizes))).astype(F)
        _d, _j, mesh = check_lattice(fi, f, sizes, 0.0, method)
        if method == "iso" and len(sizes) == 3:
            P = mesh.vertices[mesh.indices]
            assert ((P[:, 0] == P[:, 1]).all(1) | (P[:, 1] == P[:, 2]).all(1) | (P[:, 0] == P[:, 2]).all(1)).any()


def check_queries(fi, mesh, sizes, rng, n=1000):
    """off-lattice and non-finite queries against a mesh: distances, primitives, closest points"""
    D = len(sizes)
    q = np.stack([rng.uniform(-3, s + 2, n) for s in sizes], 1).astype(F)
    q[:50] = np.round(q[:50])
    q[50:60] = mesh.vertices[rng.integers(0, len(mesh.vertices), 10)]
    q[60, 0], q[61, D - 1], q[62, 0] = np.nan, np.inf, -np.inf
    s = fi.SurfaceIndex.from_mesh(mesh)
    for md in (math.inf, 1.5):
        d, j, c = s.distance(q, md, primitives=True, closest=True)
        wd, wj, wc = S.distance(mesh.vertices, mesh.indices, q, D, md)
        same_bits(d, wd)
        assert np.array_equal(j, wj)
        same_bits(c, wc)
    assert np.isnan(d[60:63]).all() and (j[60:63] == -1).all() and np.isnan(c[60:63]).all()
    assert np.array_equal(bits(s.distance(q, 1.5)), bits(d))


def check_subset(fi, xs, sizes, ctx, rng, n=1000):
    """the context's redistancing of its last solution (xs: that solution as fp32) at n random lattice points, both methods"""
    at = rng.choice(int(np.prod(sizes)), n, replace=False)
    for method in ("iso", "dual"):
        d, j, mesh = ctx.redistance(None, 0.0, method, primitives=True)
        wd, wj = S.redistance(xs, sizes, 0.0, method, at=at)
        same_bits(d[at], wd)
        assert np.array_equal(j[at], wj)
        v, i, _inside = S.surface(xs, sizes, 0.0, method)
        assert np.array_equal(bits(mesh.vertices), bits(v)) and np.array_equal(mesh.indices, i)
        assert np.array_equal(bits(ctx.redistance(None, 0.0, method)), bits(d))
    check_queries(fi, mesh, sizes, rng)


def test_random_subset_at_96(fi):
    sizes = [96, 96, 96]
    f = smooth(sizes, 5, k=0.2)
    ctx = fi.LatticeField(sizes)
    rng = np.random.default_rng(96)
    at = rng.choice(f.size, 1000, replace=False)
    for method in ("iso", "dual"):
        d, j, mesh = ctx.redistance(f, 0.0, method, primitives=True)
        wd, wj = S.redistance(f, sizes, 0.0, method, at=at)
        same_bits(d[at], wd)
        assert np.array_equal(j[at], wj)
        check_queries(fi, mesh, sizes, rng)


def test_config3_at_1024(fi):
    from field_interpolation_amd import bench_settings as bs
    from field_interpolation_amd import synth
    sizes, w, pos, nrm = synth.config3(side=1024, points_per_shape=25000, seed=2)
    f = fi.LatticeField(sizes, dtype="f64")
    f.add_field_constraints(w)
    s = bs.SETTINGS[3]   # 4096 -> 1024: two levels less, the same coarsest lattice
    bs.configure(f, s["levels"] - 2, s["coarse_tol"], kcycle=s.get("kcycle", 0), cheb=s.get("cheb"))
    f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
    f.assemble()
    f.solve_cg(None, 0, s["tol"])
    check_subset(fi, f.solution_f64().astype(F), sizes, f, np.random.default_rng(3))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_config5_shape_at_128(fi, dtype):
    from field_interpolation_amd import bench_settings as bs
    from field_interpolation_amd import synth
    sizes, w, pos, nrm = synth.config5(side=128, num_points=312500, seed=4)
    s = bs.SETTINGS[5]
    f = fi.LatticeField(sizes, dtype=dtype)
    f.add_field_constraints(w)
    # the benchmark's settings; mixed precision needs an fp64 context, so the fp32 one runs its V-cycle in fp32
    bs.configure(f, s["levels"], s["coarse_tol"], mixed=dtype == "f64", by_field=True, kcycle=s.get("kcycle", 0), cheb=s.get("cheb"))
    f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
    f.assemble()
    x, _it, _rel = f.solve_cg(None, 0 if dtype == "f64" else 200, s["tol"])
    xs = f.solution_f64().astype(F) if dtype == "f64" else x    # an fp64 solution is rounded to fp32 once
    check_subset(fi, xs, sizes, f, np.random.default_rng(5))


def test_surface_from_host_arrays_equals_from_mesh(fi):
    sizes = [40, 36, 30]
    f = smooth(sizes, 9)
    mesh = fi.iso_surface(f, sizes)
    a = fi.SurfaceIndex(mesh.vertices, mesh.indices)
    b = fi.SurfaceIndex.from_mesh(mesh)
    q = np.random.default_rng(1).uniform(-2, 42, (3000, 3)).astype(F)
    for x, y in zip(a.distance(q, primitives=True, closest=True), b.distance(q, primitives=True, closest=True)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    x, y = a.distance_field(sizes, 3.0, primitives=True), b.distance_field(sizes, 3.0, primitives=True)
    assert np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(x[1], y[1])
    assert a.distance(np.zeros((0, 3), F)).shape == (0,)


def test_repeated_calls_give_identical_bytes(fi):
    sizes = [64, 60, 56]
    f = smooth(sizes, 12)
    for method in ("iso", "dual"):
        a = fi.redistance(f, sizes, 0.0, method)
        b = fi.redistance(f, sizes, 0.0, method)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_empty_meshes_give_infinities(fi):
    for sizes in ([9, 8], [6, 5, 4], [1, 7, 7], [5, 1]):
        n = int(np.prod(sizes))
        for method in ("iso", "dual"):
            assert np.all(fi.redistance(np.ones(n, F), sizes, 0.0, method) == np.inf)
            assert np.all(fi.redistance(-np.ones(n, F), sizes, 0.0, method) == -np.inf)
    s = fi.SurfaceIndex(np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    d, j, c = s.distance(np.ones((5, 3), F), primitives=True, closest=True)
    assert np.all(d == np.inf) and np.all(j == -1) and np.isnan(c).all()


def test_analytic_sphere_at_128(fi):
    sizes = [128, 128, 128]
    p = lattice_points(sizes).astype(np.float64)
    centre = np.array([63.7, 64.2, 63.4])
    radius = 40.0
    exact = np.linalg.norm(p - centre, axis=1) - radius
    d = fi.redistance(exact.astype(F), sizes).astype(np.float64)
    err = np.abs(d - exact)
    print("max |d - exact| =", err.max())
    assert err.max() <= 0.05
    g = d.reshape(sizes[::-1])
    grad = np.zeros(g.shape)
    for ax in range(3):
        diff = np.full(g.shape, np.nan)
        sl = [slice(None)] * 3
        lo, hi, mid = list(sl), list(sl), list(sl)
        lo[ax], hi[ax], mid[ax] = slice(0, -2), slice(2, None), slice(1, -1)
        diff[tuple(mid)] = (g[tuple(hi)] - g[tuple(lo)]) / 2
        grad += diff ** 2
    grad = np.sqrt(grad).reshape(-1)
    # >= 2 units from the surface and >= 6 from the centre: nearer the centre the central difference itself is off (on the
    # exact signed distance by 0.069 at 2 units, 0.019 at 4, 0.009 at 6; measured on the CPU)
    ok = (np.abs(exact) >= 2) & (np.linalg.norm(p - centre, axis=1) >= 6) & np.isfinite(grad)
    print("|grad d| in", grad[ok].min(), grad[ok].max())
    assert np.all(np.abs(grad[ok] - 1) <= 0.02)


def test_errors(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    sizes = [8, 7, 6]
    f = smooth(sizes, 2)
    out = np.empty(f.size, F)
    sz = (C.c_int * 3)(*sizes)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def code(fn):
        with pytest.raises(fi.FiError) as e:
            fn()
        return e.value.code

    v = np.zeros((4, 3), F)
    assert code(lambda: fi.SurfaceIndex(v, np.array([[0, 1, 4]], np.int32))) == 1
    assert code(lambda: fi.SurfaceIndex(v, np.array([[0, -1, 2]], np.int32))) == 1
    assert code(lambda: fi.SurfaceIndex(np.zeros((4, 1), F), np.array([[0]], np.int32))) == 5
    s = fi.SurfaceIndex(v, np.array([[0, 1, 2]], np.int32))
    q = np.zeros((3, 3), F)
    assert code(lambda: s.distance(q, float("nan"))) == 1
    assert code(lambda: s.distance(q, -1.0)) == 1
    assert code(lambda: s.distance_field(sizes, -1.0)) == 1
    d = np.empty(3, F)
    h = C.c_void_p()
    assert L.fi_surface_distance(s._h, -1, ptr(q), C.c_float(1.0), ptr(d), None, None, 0) == 1
    assert L.fi_surface_distance(s._h, 3, None, C.c_float(1.0), ptr(d), None, None, 0) == 1
    assert L.fi_surface_distance(s._h, 1 << 31, ptr(q), C.c_float(1.0), ptr(d), None, None, 0) == 5
    assert L.fi_surface_distance(s._h, 0, ptr(q), C.c_float(1.0), ptr(d), None, None, 0) == 0
    assert L.fi_surface_create(C.byref(h), 3, 4, ptr(v), 1 << 31, ptr(np.zeros(3, np.int32)), 0) == 5
    assert L.fi_surface_create(C.byref(h), 3, 4, None, 1, ptr(np.zeros(3, np.int32)), 0) == 1
    assert L.fi_redistance_field(ptr(f), 3, sz, C.c_float(0), 7, C.c_float(np.inf), ptr(out), None, None, 0) == 1
    assert L.fi_redistance_field(ptr(f), 3, sz, C.c_float(0), 0, C.c_float(np.nan), ptr(out), None, None, 0) == 1
    assert L.fi_redistance_field(ptr(f), 3, sz, C.c_float(0), 0, C.c_float(np.inf), None, None, None, 0) == 1
    assert L.fi_redistance_field(ptr(f), 1, sz, C.c_float(0), 0, C.c_float(np.inf), ptr(out), None, None, 0) == 5
    assert L.fi_redistance_field(ptr(f), 4, sz, C.c_float(0), 0, C.c_float(np.inf), ptr(out), None, None, 0) == 5
    with pytest.raises(ValueError):
        fi.redistance(f, sizes, method="marching")
    bad = f.copy()
    bad[17] = np.nan
    for method in ("iso", "dual"):
        assert code(lambda: fi.redistance(bad, sizes, 0.0, method)) == 1
    ctx = fi.LatticeField(sizes)
    assert code(lambda: ctx.redistance()) == 3                          # no solution yet
    assert code(lambda: fi.LatticeField([20]).redistance(np.zeros(20, F))) == 5
    g = fi.LatticeGroup([16, 16, 16], nranks=2)
    r0 = g.members[0]
    assert code(lambda: r0.redistance(np.zeros(r0.num_owned, F))) == 5
