"""Normal orientation on the device (fi_orient.hip through fi_orient_normals and fi_points_orient_normals) against the numpy
restatement of the contract (tests/orient_reference.py orient_normals): normals as bit patterns and components exactly, in
2-D and 3-D, on generic and degenerate clouds, with estimated and with random normals, for every anchor; clouds of many
components, long hook chains, several workgroups; dead points; repeatability; device tensors; the error codes; and the
pipeline scan -> normals -> oriented points -> SDF without a guide."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import normals_reference as R
import orient_reference as O
from test_gpu_normals import CLOUDS, KS, N, SIZES, _cloud
from util import sphere_points

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _bits(a):
    return np.ascontiguousarray(np.asarray(a), np.float32).view(np.uint32)


def _same(got, want, what=""):
    gn, gc = np.asarray(got[0]), np.asarray(got[1])
    wn, wc = want
    assert gn.dtype == np.float32 and gc.dtype == np.int64 and gn.shape == wn.shape and gc.shape == wc.shape
    bad = np.flatnonzero(gc != wc)
    assert bad.size == 0, (what, "components", bad.size, bad[:5], gc[bad[:5]], wc[bad[:5]])
    bad = np.flatnonzero(np.any(_bits(gn) != _bits(wn), axis=1))
    assert bad.size == 0, (what, "normals", bad.size, bad[:5], gn[bad[:5]], wn[bad[:5]])


def _check(index, pos, nrm, D, k, nb=None, md=math.inf, what="", **guides):
    want = O.orient_normals(pos, nrm, D, k, md, neighbours=nb, **guides)
    before = nrm.copy()
    _same(index.orient_normals(nrm, k=k, max_distance=md, components=True, **guides), want, what)
    assert np.array_equal(_bits(nrm), _bits(before))                   # the Python entry works on a copy
    return want


@functools.lru_cache(maxsize=None)
def _neighbours(D, kind):
    rng = np.random.default_rng(100 * D + CLOUDS.index(kind))
    pos = _cloud(rng, kind, SIZES[D])
    nb = R.knn(pos, pos, D, 32)
    pos.setflags(write=False)
    return pos, nb


@pytest.mark.parametrize("normals", ["estimated", "random"])
@pytest.mark.parametrize("kind", CLOUDS)
@pytest.mark.parametrize("D", [2, 3], ids=["2D", "3D"])
def test_matches_the_restatement(fi, D, kind, normals):
    pos, nb = _neighbours(D, kind)
    pi = fi.PointIndex(pos, ndim=D)
    rng = np.random.default_rng(7)
    comps = []
    for k in KS:
        nbk = (nb[0][:, :k], nb[1][:, :k])                             # (a smaller k is a prefix of a larger one's result)
        if normals == "estimated":                                     # (on the degenerate clouds: zero normals, ties in a)
            nrm = pi.estimate_normals(k=k)
        else:                                                          # dense flips, every a different
            nrm = rng.normal(size=(N, D)).astype(np.float32)
        comps.append(np.unique(_check(pi, pos, nrm, D, k, nbk, what=(k, normals))[1]).size)
    print(D, kind, normals, "components at k = 3, 8, 16, 32:", comps)


@functools.lru_cache(maxsize=None)
def _sphere(n, k, noise=0.05, seed=5):
    pos, _ = sphere_points(np.random.default_rng(seed), SIZES[3], n, noise=noise)
    nb = R.knn(pos, pos, 3, k)
    nrm = R.estimate_normals(pos, 3, max(k, 3), neighbours=nb)[0] if k >= 3 else None
    pos.setflags(write=False)
    return pos, nb, nrm


@pytest.mark.parametrize("n", [4000, 600])
def test_hundreds_of_components(fi, n):
    pos, nb, nrm = _sphere(n, 3)
    want = _check(fi.PointIndex(pos), pos, nrm, 3, 3, nb)
    count = np.unique(want[1]).size
    print("components:", count)
    assert count > (100 if n == 4000 else 15)


def test_two_spheres_apart(fi):
    a, nb, na = _sphere(600, 8, noise=0.0, seed=3)
    pos = np.concatenate([a, a + np.float32([40.0, 0, 0])])
    nrm = np.concatenate([na, -na]).astype(np.float32)
    pi = fi.PointIndex(pos)
    want = _check(pi, pos, nrm, 3, 8, md=6.0)
    assert sorted(np.unique(want[1]).tolist()) == [0, 600]
    centre = (np.array(SIZES[3], np.float32) - 1) / 2
    out = np.sum(want[0][:600] * (a - centre), axis=1) > 0
    assert out.all() and np.array_equal(_bits(want[0][600:]), _bits(want[0][:600]))   # both outward, whatever came in
    # one viewpoint between them: each sphere votes on its own (so near, it sees the smaller part of either)
    _check(pi, pos, nrm, 3, 8, md=6.0, viewpoints=np.float32([[25.0, 8.5, 7.5]]))


def test_spiral_long_hook_chains(fi):
    """a 2-D spiral whose normals turn slowly: at k = 2 every point lists its predecessor or successor, and a round hooks
    long chains of components onto one another, so that the pointer jumping is deep"""
    t = np.linspace(0.0, 1.0, N)
    r, ang = 2.0 + 16.0 * t, 12.0 * np.pi * np.sqrt(t)
    pos = np.stack([20 + r * np.cos(ang), 15 + r * np.sin(ang)], 1).astype(np.float32)
    nrm = np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
    nrm[::3] = -nrm[::3]
    pi = fi.PointIndex(pos)
    want = _check(pi, pos, nrm, 2, 2)
    print("components:", np.unique(want[1]).size)
    perm = np.random.default_rng(3).permutation(N)                     # and with the chain scattered over the indices
    _check(fi.PointIndex(pos[perm]), pos[perm], nrm[perm], 2, 2)


def test_several_workgroups_and_more_rounds(fi):
    """12 000 points.  (The brute-force neighbour search of the restatement alone would take ten seconds here: the
    neighbours and the normals it starts from are the device's, which test_gpu_knn.py and test_gpu_normals.py hold to their
    own restatements bit for bit; every other test of this file searches on its own.)"""
    pos, _ = sphere_points(np.random.default_rng(5), SIZES[3], 12000, noise=0.05)
    pi = fi.PointIndex(pos)
    want = _check(pi, pos, pi.estimate_normals(k=16), 3, 16, pi.knn(pos, 16))
    assert np.unique(want[1]).size == 1


def test_one_and_two_points(fi):
    one = np.float32([[3.0, 4.0, 5.0]])
    for nrm in (np.float32([[0.0, 0.0, -2.0]]), np.float32([[0.0, -1.0, 0.0]]), np.float32([[0.0, 0.0, 0.0]])):
        _check(fi.PointIndex(one), one, nrm, 3, 4)
    got = fi.PointIndex(one).orient_normals(np.float32([[0.0, -1.0, 0.0]]), k=1)
    assert np.array_equal(_bits(got), _bits(np.float32([[-0.0, 1.0, -0.0]])))            # by hand: axis 2 is zero, axis 1 decides
    two = np.float32([[1.0, 1.0], [2.0, 3.0]])
    for k in (1, 2, 32):
        for nrm in (np.float32([[1, 0], [-1, 0.5]]), np.float32([[0, -1], [0, -1]]), np.float32([[1, 1], [0, 0]])):
            _check(fi.PointIndex(two), two, nrm, 2, k)
    got, comp = fi.PointIndex(two).orient_normals(np.float32([[1, 0], [-1, 0.5]]), k=2, components=True)
    # by hand: one edge, d = -1: t = (+, -); point 1 is higher, t_1 n_1 = (1, -0.5) looks down: S = -1
    assert np.array_equal(_bits(got), _bits(np.float32([[-1, -0.0], [-1, 0.5]]))) and comp.tolist() == [0, 0]
    got, comp = fi.PointIndex(two).orient_normals(np.float32([[1, 0], [-1, 0.5]]), k=1, components=True)
    # k = 1: every point lists itself alone: no edges; n_0 = (1, 0) stays, n_1 = (-1, 0.5) looks up and stays
    assert np.array_equal(_bits(got), _bits(np.float32([[1, 0], [-1, 0.5]]))) and comp.tolist() == [0, 1]


@pytest.mark.parametrize("D", [2, 3], ids=["2D", "3D"])
def test_dead_points_keep_their_bits(fi, D):
    rng = np.random.default_rng(40 + D)
    pos = _cloud(rng, "random", SIZES[D])
    nrm = rng.normal(size=(N, D)).astype(np.float32)
    pos[::41, 0] = np.nan
    pos[5::97, D - 1] = np.inf
    nrm[3::50] = 0.0
    nrm[9::70] = -0.0
    nrm[11::83, D - 1] = np.nan
    nrm[13::89, 0] = -np.inf
    pi = fi.PointIndex(pos, ndim=D)
    nb = R.knn(pos, pos, D, 16)
    for k in (4, 16):
        want = _check(pi, pos, nrm, D, k, (nb[0][:, :k], nb[1][:, :k]))
        dead = want[1] < 0
        assert dead.sum() > 250 and np.array_equal(_bits(want[0][dead]), _bits(nrm[dead]))
    md = 0.45 if D == 2 else 0.9                                       # and points without any neighbour within reach
    want = _check(pi, pos, nrm, D, 16, md=md)
    assert np.unique(want[1]).size > 20


@pytest.mark.parametrize("k", [3, 16])
@pytest.mark.parametrize("D", [2, 3], ids=["2D", "3D"])
def test_votes(fi, D, k):
    """both vote anchors, one guide and one per point, guides with zeros and NaNs, over many components (k = 3) and over
    one (k = 16)"""
    pos, nb = _neighbours(D, "sphere")
    sizes = SIZES[D]
    rng = np.random.default_rng(60 + D)
    nrm = R.estimate_normals(pos, D, 16, neighbours=(nb[0][:, :16], nb[1][:, :16]))[0]
    centre = (np.array(sizes, np.float32) - 1) / 2
    one = (centre + np.float32(100.0) * np.eye(D, dtype=np.float32)[0]).reshape(1, D)
    per_point = (centre + 2 * (pos - centre)).astype(np.float32)
    per_point[::50] = pos[::50]                                        # w == 0
    per_point[7::90, 0] = np.nan
    rough = rng.normal(size=(N, D)).astype(np.float32)
    rough[::50] = 0.0
    rough[7::90, 0] = np.nan
    pi = fi.PointIndex(pos, ndim=D)
    nbk = (nb[0][:, :k], nb[1][:, :k])
    plain = _check(pi, pos, nrm, D, k, nbk)
    differ = 0
    for name, kw in (("one viewpoint", {"viewpoints": one}), ("centre", {"viewpoints": centre.reshape(1, D)}),
                     ("n viewpoints", {"viewpoints": per_point}), ("directions", {"directions": rough}),
                     ("all NaN", {"directions": np.full((N, D), np.nan, np.float32)})):
        want = _check(pi, pos, nrm, D, k, nbk, what=(k, name), **kw)
        assert np.array_equal(want[1], plain[1])
        differ += int(not np.array_equal(_bits(want[0]), _bits(plain[0])))
        if name == "all NaN":
            assert np.array_equal(_bits(want[0]), _bits(plain[0]))
    assert differ >= 1                                                 # the votes do decide


@pytest.mark.parametrize("D", [2, 3], ids=["2D", "3D"])
def test_a_tied_vote_falls_back_on_the_extreme_rule(fi, D):
    # two points, the directions say + for one and - for the other; the extreme rule decides
    two = np.zeros((2, D), np.float32)
    two[1, 0] = 1.0
    n2 = np.zeros((2, D), np.float32)
    n2[:, D - 1] = [-1.0, -2.0]
    g = np.zeros((2, D), np.float32)
    g[:, D - 1] = [1.0, -1.0]
    got = fi.PointIndex(two, ndim=D).orient_normals(n2, k=2, directions=g)
    assert np.array_equal(_bits(got), _bits(-n2))                      # by hand: t = (+, +), both look down: S = -1
    _check(fi.PointIndex(two, ndim=D), two, n2, D, 2, directions=g)
    g[1, D - 1] = 1.0                                                  # w = -1, -2: two votes -, S = -1 without the rule
    _check(fi.PointIndex(two, ndim=D), two, n2, D, 2, directions=g)
    g[:, D - 1] = -1.0                                                 # two votes +: nothing turns
    assert np.array_equal(_bits(fi.PointIndex(two, ndim=D).orient_normals(n2, k=2, directions=g)), _bits(n2))


def test_repeatable_and_the_context_entry(fi):
    sizes = SIZES[3]
    rng = np.random.default_rng(23)
    a, b = sphere_points(rng, sizes, 2500)[0], _cloud(rng, "random", sizes, 1500)
    pos = np.concatenate([a, b])
    nrm = rng.normal(size=(N, 3)).astype(np.float32)
    view = np.array([[-50.0, 9.0, 8.0]], np.float32)
    pi = fi.PointIndex(pos)
    first = pi.orient_normals(nrm, k=10, viewpoints=view, components=True)
    _same(first, O.orient_normals(pos, nrm, 3, 10, viewpoints=view))
    _same(pi.orient_normals(nrm, k=10, viewpoints=view, components=True), first, "the same call twice")
    _same(fi.PointIndex(pos).orient_normals(nrm, k=10, viewpoints=view, components=True), first, "a rebuilt index")
    assert np.array_equal(_bits(pi.orient_normals(nrm, k=10, viewpoints=view)), _bits(first[0]))   # components are optional
    f = fi.LatticeField(sizes)
    f.add_field_constraints(fi.Weights())
    f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, a)
    f.add_border_prior(0.5)                                          # lattice points, not data
    f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, b)
    _same(f.orient_normals(nrm, k=10, viewpoints=view, components=True), first, "the context entry")
    # estimate_normals(propagate=True) is the two calls in a row, the guides as votes
    est = pi.estimate_normals(k=10)
    want = pi.orient_normals(est, k=10, viewpoints=view)
    got, var = pi.estimate_normals(k=10, viewpoints=view, variation=True, propagate=True)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(var.view(np.uint32), pi.estimate_normals(k=10, variation=True)[1].view(np.uint32))
    assert np.array_equal(_bits(f.estimate_normals(k=10, viewpoints=view, propagate=True)), _bits(want))


def test_device_tensors(tmp_path):
    """torch device tensors as normals and guides: torch device tensors out, equal to the restatement; in a fresh process
    (tests/orient_torch_worker.py), as torch must stay out of this one"""
    import os
    import subprocess
    import sys
    sizes = [30, 26, 22]
    rng = np.random.default_rng(8)
    pos, _ = sphere_points(rng, sizes, 3000)
    nrm = rng.normal(size=(3000, 3)).astype(np.float32)
    nrm[::40] = 0.0
    view = np.array([[14.5, 12.5, 60.0]], np.float32)
    np.savez(tmp_path / "in.npz", sizes=np.array(sizes), pos=pos, nrm=nrm, k=np.array([12]), view=view)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "orient_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"].all() and o["input_untouched"].all()
    want = O.orient_normals(pos, nrm, 3, 12, viewpoints=view)
    _same((o["ctx_n"], o["ctx_c"]), want, "context")
    _same((o["pts_n"], o["pts_c"]), want, "point set")
    _same((o["host_guides_n"], o["pts_c"]), want, "host guides, device=True")
    plain = O.orient_normals(pos, nrm, 3, 12)
    _same((o["plain_n"], o["plain_c"]), plain, "no guides")


def test_error_codes(fi):
    from field_interpolation_amd import _capi
    L = _capi.lib()
    pos = np.random.default_rng(1).uniform(0, 9, size=(40, 3)).astype(np.float32)
    f = fi.LatticeField([10, 10, 10])
    f.add_field_constraints(fi.Weights())
    f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, pos)
    nrm = np.ones((40, 3), np.float32)
    comp = np.empty(40, np.int64)
    g = np.ones((40, 3), np.float32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    inf = math.inf
    assert L.fi_orient_normals(f._h, 8, inf, 0, None, 0, ptr(nrm), ptr(comp), 0) == 0
    assert L.fi_orient_normals(f._h, 1, inf, 0, None, 0, ptr(nrm), None, 0) == 0          # k = 1 and 2 are fine here
    assert L.fi_orient_normals(f._h, 2, inf, 0, None, 0, ptr(nrm), None, 0) == 0
    assert L.fi_orient_normals(f._h, 0, inf, 0, None, 0, ptr(nrm), None, 0) == 1
    assert L.fi_orient_normals(f._h, 33, inf, 0, None, 0, ptr(nrm), None, 0) == 1
    assert L.fi_orient_normals(f._h, 8, inf, 0, None, 0, None, None, 0) == 1
    assert L.fi_orient_normals(f._h, 8, -1.0, 0, None, 0, ptr(nrm), None, 0) == 1
    assert L.fi_orient_normals(f._h, 8, math.nan, 0, None, 0, ptr(nrm), None, 0) == 1
    assert L.fi_orient_normals(f._h, 8, inf, 3, ptr(g), 40, ptr(nrm), None, 0) == 1       # no such anchor
    assert L.fi_orient_normals(f._h, 8, inf, -1, ptr(g), 40, ptr(nrm), None, 0) == 1
    assert L.fi_orient_normals(f._h, 8, inf, 1, None, 40, ptr(nrm), None, 0) == 1         # an anchor without guides
    assert L.fi_orient_normals(f._h, 8, inf, 1, ptr(g), 39, ptr(nrm), None, 0) == 1       # a wrong count
    assert L.fi_orient_normals(f._h, 8, inf, 2, ptr(g), 1, ptr(nrm), None, 0) == 1        # directions: one per point
    assert L.fi_orient_normals(f._h, 8, inf, 1, ptr(g), 1, ptr(nrm), None, 0) == 0
    assert L.fi_orient_normals(f._h, 8, inf, 2, ptr(g), 40, ptr(nrm), None, 0) == 0
    assert L.fi_orient_normals(f._h, 8, inf, 0, None, 0, ptr(nrm), None, 5) == 1
    assert L.fi_orient_normals(None, 8, inf, 0, None, 0, ptr(nrm), None, 0) == 1
    out = np.empty((40, 3), np.float32)
    assert L.fi_estimate_normals(f._h, 8, inf, 3, ptr(g), 40, ptr(out), None, 0) == 1     # still no such mode there
    h = C.c_void_p()
    assert L.fi_points_create(C.byref(h), 1, 40, ptr(pos), 0) == 0
    try:
        assert L.fi_points_orient_normals(h, 8, inf, 0, None, 0, ptr(nrm), None, 0) == 1  # 1-D: no normals
    finally:
        L.fi_points_destroy(h)
    assert L.fi_points_orient_normals(None, 8, inf, 0, None, 0, ptr(nrm), None, 0) == 1
    with pytest.raises(ValueError):
        f.orient_normals(nrm, viewpoints=g, directions=g)
    with pytest.raises(ValueError):
        f.orient_normals(nrm[:39])
    empty = fi.PointIndex(np.zeros((0, 3), np.float32))
    got, c = empty.orient_normals(np.zeros((0, 3), np.float32), components=True)           # n = 0 is a success
    assert got.shape == (0, 3) and c.shape == (0,)
    s = fi.LatticeField([12, 10, 16], dtype="f32", rank=1, nranks=2)                       # a slab context
    s.add_field_constraints(fi.Weights())
    s.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, np.array([[3.0, 4.0, 9.0]], np.float32))
    with pytest.raises(fi.FiError) as e:
        s.orient_normals(np.ones((1, 3), np.float32), k=8)
    assert e.value.code == 5


def test_scan_to_signed_distance_field_without_a_guide(fi):
    sizes = SIZES[3]
    pos, _ = sphere_points(np.random.default_rng(1), sizes, N, noise=0.0)
    centre = ((np.array(sizes) - 1) / 2.0).astype(np.float32)
    nb = R.knn(pos, pos, 3, 16)
    canonical = R.estimate_normals(pos, 3, 16, neighbours=nb)[0]
    want, comp = O.orient_normals(pos, canonical, 3, 16, neighbours=nb)
    assert np.all(np.sum(want.astype(np.float64) * (pos - centre), axis=1) > 0)          # the restatement: 100 % outward
    view = (centre + 2 * (pos - centre)).astype(np.float32)
    pi = fi.PointIndex(pos)
    got = pi.estimate_normals(k=16, propagate=True)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got), _bits(pi.estimate_normals(k=16, viewpoints=view)))
    w = fi.Weights()
    f = fi.sdf_from_unoriented_points(sizes, w, pos, k=16, propagate=True)
    g = fi.sdf_from_points(sizes, w, pos, got)
    x = [fi.solve_sparse_linear_with_guess(h, np.zeros(h.num_unknowns, np.float32), 300, 1e-5) for h in (f, g)]
    assert x[0] is not None and np.array_equal(x[0], x[1])
    field = np.asarray(x[0]).reshape(sizes[2], sizes[1], sizes[0])    # (z, y, x)
    assert field[sizes[2] // 2, sizes[1] // 2, sizes[0] // 2] < 0
    for z in (0, -1):
        for y in (0, -1):
            for xx in (0, -1):
                assert field[z, y, xx] > 0
