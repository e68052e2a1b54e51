"""Point-cloud normals on the device (fi_knn.hip through fi_estimate_normals and fi_points_estimate_normals) against the
numpy restatement of the contract (tests/normals_reference.py estimate_normals): normals and surface variation bit for bit,
in 2-D and 3-D, on generic and degenerate clouds, for every kernel class, every orientation mode and a max_distance that
leaves points without a plane; the context entry against the PointIndex entry; input order; device tensors; the error
codes; and sdf_from_unoriented_points against the sequence by hand."""
import ctypes as C
import math

import numpy as np
import pytest

import normals_reference as R
from util import sphere_points

pytestmark = pytest.mark.gpu

N = 4000
KS = [3, 8, 16, 32]


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _same(got, want, what=""):
    gn, gv = np.asarray(got[0]), np.asarray(got[1])
    wn, wv = want
    assert gn.dtype == np.float32 and gv.dtype == np.float32 and gn.shape == wn.shape and gv.shape == wv.shape
    bad = np.flatnonzero(np.any(gn.view(np.uint32) != wn.view(np.uint32), axis=1))
    assert bad.size == 0, (what, bad.size, bad[:5], gn[bad[:5]], wn[bad[:5]])
    assert np.array_equal(np.isnan(gv), np.isnan(wv)), what
    bad = np.flatnonzero((gv.view(np.uint32) != wv.view(np.uint32)) & ~np.isnan(wv))
    assert bad.size == 0, (what, bad.size, bad[:5], gv[bad[:5]], wv[bad[:5]])


CLOUDS = ["random", "sphere", "plane", "collinear", "identical", "grid ties"]
SIZES = {2: [40, 30], 3: [20, 18, 16]}


def _cloud(rng, kind, sizes, n=N):
    D = len(sizes)
    if kind == "random":
        return np.stack([rng.uniform(-2, s + 1, n) for s in sizes], 1).astype(np.float32)
    if kind == "sphere":
        return sphere_points(rng, sizes, n, noise=0.05)[0]
    if kind == "plane":                                              # the last coordinate is 7 exactly
        p = np.stack([rng.uniform(0, s - 1, n) for s in sizes], 1).astype(np.float32)
        p[:, D - 1] = 7.0
        return p
    if kind == "collinear":
        t = rng.uniform(0, 1, n).astype(np.float32)
        return (np.outer(t, np.array(sizes, np.float32) - 1)).astype(np.float32)
    if kind == "identical":
        return np.tile(np.float32(np.array(sizes) / 3.0), (n, 1)).astype(np.float32)
    return rng.integers(0, 8, size=(n, D)).astype(np.float32)        # many exact ties


@pytest.mark.parametrize("kind", CLOUDS)
@pytest.mark.parametrize("D", [2, 3], ids=["2D", "3D"])
def test_matches_the_restatement(fi, D, kind):
    sizes = SIZES[D]
    rng = np.random.default_rng(100 * D + CLOUDS.index(kind))
    pos = _cloud(rng, kind, sizes)
    centre = (np.array(sizes, np.float32) - 1) / 2
    one = (centre + np.float32(100.0) * np.eye(D, dtype=np.float32)[0]).reshape(1, D)
    per_point = (centre + 2 * (pos - centre)).astype(np.float32)
    rough = rng.normal(size=(N, D)).astype(np.float32)
    rough[::50] = 0.0                                                # w == 0: the canonical sign stays
    rough[7::90, 0] = np.nan                                         # a non-finite w too
    nb = R.knn(pos, pos, D, 32)
    pi = fi.PointIndex(pos, ndim=D)
    for k in [k for k in KS if k >= D]:
        nbk = (nb[0][:, :k], nb[1][:, :k])                           # (a smaller k is a prefix of a larger one's result)
        for name, kw in (("canonical", {}), ("one viewpoint", {"viewpoints": one}), ("n viewpoints", {"viewpoints": per_point}),
                         ("directions", {"directions": rough})):
            want = R.estimate_normals(pos, D, k, neighbours=nbk, **kw)
            _same(pi.estimate_normals(k=k, variation=True, **kw), want, (k, name))
    assert np.array_equal(pi.estimate_normals(k=16), pi.estimate_normals(k=16, variation=True)[0])   # variation is optional


@pytest.mark.parametrize("D", [2, 3], ids=["2D", "3D"])
def test_max_distance_leaves_points_without_a_plane(fi, D):
    sizes = SIZES[D]
    rng = np.random.default_rng(17 + D)
    pos = _cloud(rng, "random", sizes)
    pos[::41, 0] = np.nan                                            # and non-finite points: zero normals too
    pos[5::97, D - 1] = np.inf
    md = 0.45 if D == 2 else 0.9
    pi = fi.PointIndex(pos, ndim=D)
    for k in (8, 32):
        want = R.estimate_normals(pos, D, k, max_distance=md, viewpoints=np.zeros((1, D), np.float32))
        none = np.isnan(want[1])
        assert none.sum() > N // 10 and (~none).sum() > N // 10       # both kinds are there
        assert np.all(want[0][none] == 0)
        _same(pi.estimate_normals(k=k, max_distance=md, viewpoints=np.zeros((1, D), np.float32), variation=True), want, k)


def test_the_context_entry_equals_the_point_set_entry(fi):
    sizes = SIZES[3]
    rng = np.random.default_rng(23)
    a, b = sphere_points(rng, sizes, 2500)[0], _cloud(rng, "random", sizes, 1500)
    f = fi.LatticeField(sizes)
    f.add_field_constraints(fi.Weights())
    f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, a)
    f.add_border_prior(0.5)                                          # lattice points, not data
    f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, b)
    pos = np.concatenate([a, b])
    view = np.array([[-50.0, 9.0, 8.0]], np.float32)
    want = fi.PointIndex(pos).estimate_normals(k=10, viewpoints=view, variation=True)
    _same(f.estimate_normals(k=10, viewpoints=view, variation=True), want)
    _same(want, R.estimate_normals(pos, 3, 10, viewpoints=view))


def test_input_order_is_kept(fi):
    sizes = SIZES[3]
    rng = np.random.default_rng(29)
    pos = _cloud(rng, "random", sizes)
    perm = rng.permutation(N)
    n0, v0 = fi.PointIndex(pos).estimate_normals(k=12, variation=True)
    n1, v1 = fi.PointIndex(pos[perm]).estimate_normals(k=12, variation=True)
    d = R.knn(pos, pos, 3, 12)[0]
    distinct = np.all(np.diff(d, axis=1) > 0, axis=1)                # no ties: the neighbour ORDER does not depend on indices
    assert distinct.mean() > 0.9
    keep = distinct[perm]
    assert np.array_equal(n1[keep].view(np.uint32), n0[perm][keep].view(np.uint32))
    assert np.array_equal(v1[keep].view(np.uint32), v0[perm][keep].view(np.uint32))


def test_device_tensors(tmp_path):
    """torch device tensors as viewpoints: torch device tensors out, equal to the restatement; in a fresh process
    (tests/knn_torch_worker.py), as torch must stay out of this one"""
    import os
    import subprocess
    import sys
    sizes = [30, 26, 22]
    rng = np.random.default_rng(8)
    pos, _ = sphere_points(rng, sizes, 3000)
    view = np.array([[14.5, 12.5, 10.5]], np.float32)
    np.savez(tmp_path / "in.npz", sizes=np.array(sizes), pos=pos, q=pos[:10], k=np.array([12]), view=view)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "knn_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["normals_on_device"][0] and o["plain_on_device"][0]
    want = R.estimate_normals(pos, 3, 12, viewpoints=view)
    _same((o["ctx_n"], o["ctx_v"]), want)
    _same((o["pts_n"], o["pts_v"]), want)
    assert np.array_equal(o["pts_n_plain"].view(np.uint32), R.estimate_normals(pos, 3, 12)[0].view(np.uint32))


def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    pos = np.random.default_rng(1).uniform(0, 9, size=(40, 3)).astype(np.float32)
    f = fi.LatticeField([10, 10, 10])
    f.add_field_constraints(fi.Weights())
    f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, pos)
    out = np.empty((40, 3), np.float32)
    g = np.ones((40, 3), np.float32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    inf = math.inf
    assert L.fi_estimate_normals(f._h, 8, inf, 0, None, 0, ptr(out), None, 0) == 0
    assert L.fi_estimate_normals(f._h, 2, inf, 0, None, 0, ptr(out), None, 0) == 1       # k < D
    assert L.fi_estimate_normals(f._h, 33, inf, 0, None, 0, ptr(out), None, 0) == 1
    assert L.fi_estimate_normals(f._h, 8, inf, 0, None, 0, None, None, 0) == 1
    assert L.fi_estimate_normals(f._h, 8, -1.0, 0, None, 0, ptr(out), None, 0) == 1
    assert L.fi_estimate_normals(f._h, 8, math.nan, 0, None, 0, ptr(out), None, 0) == 1
    assert L.fi_estimate_normals(f._h, 8, inf, 3, ptr(g), 40, ptr(out), None, 0) == 1    # no such mode
    assert L.fi_estimate_normals(f._h, 8, inf, 1, None, 40, ptr(out), None, 0) == 1      # a mode without guides
    assert L.fi_estimate_normals(f._h, 8, inf, 1, ptr(g), 39, ptr(out), None, 0) == 1    # a wrong count
    assert L.fi_estimate_normals(f._h, 8, inf, 2, ptr(g), 1, ptr(out), None, 0) == 1     # directions: one per point
    assert L.fi_estimate_normals(f._h, 8, inf, 1, ptr(g), 1, ptr(out), None, 0) == 0
    assert L.fi_estimate_normals(f._h, 8, inf, 2, ptr(g), 40, ptr(out), None, 0) == 0
    assert L.fi_estimate_normals(f._h, 8, inf, 0, None, 0, ptr(out), None, 5) == 1
    h = C.c_void_p()
    assert L.fi_points_create(C.byref(h), 1, 40, ptr(pos), 0) == 0
    try:
        assert L.fi_points_estimate_normals(h, 8, inf, 0, None, 0, ptr(out), None, 0) == 1   # 1-D: no normals
    finally:
        L.fi_points_destroy(h)
    assert L.fi_points_estimate_normals(None, 8, inf, 0, None, 0, ptr(out), None, 0) == 1
    with pytest.raises(ValueError):
        f.estimate_normals(viewpoints=g, directions=g)
    assert fi.PointIndex(np.zeros((0, 3), np.float32)).estimate_normals().shape == (0, 3)
    s = fi.LatticeField([12, 10, 16], dtype="f32", rank=1, nranks=2)     # a slab context
    s.add_field_constraints(fi.Weights())
    s.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, np.array([[3.0, 4.0, 9.0]], np.float32))
    with pytest.raises(fi.FiError) as e:
        s.estimate_normals(k=8)
    assert e.value.code == 5


def test_sdf_from_unoriented_points(fi):
    sizes = [24, 24, 24]
    pos, _ = sphere_points(np.random.default_rng(12), sizes, 6000, noise=0.05)
    centre = np.full((1, 3), 11.5, np.float32)
    view = (centre + 2 * (pos - centre)).astype(np.float32)          # a sensor outside, beyond each point
    w = fi.Weights()
    f = fi.sdf_from_unoriented_points(sizes, w, pos, k=16, viewpoints=view)
    nrm = fi.PointIndex(pos).estimate_normals(k=16, viewpoints=view)
    assert np.all(np.sum(nrm * (pos - centre), axis=1) > 0)          # outward
    g = fi.sdf_from_points(sizes, w, pos, nrm)
    x = [fi.solve_sparse_linear_with_guess(h, np.zeros(h.num_unknowns, np.float32), 300, 1e-5) for h in (f, g)]
    assert x[0] is not None and np.array_equal(x[0], x[1])
    field = np.asarray(x[0]).reshape(24, 24, 24)                     # (z, y, x)
    assert field[12, 12, 12] < 0 < field[0, 0, 0]
