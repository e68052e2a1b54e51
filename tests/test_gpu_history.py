"""Answers must not depend on what the process ran before.

The library keeps state between calls and between contexts on purpose ("what a buffer may hold"): the
device blocks, streams and pinned buffers of destroyed contexts serve the next one, a context keeps its vectors across solves
and re-assemblies, a buffer that shrinks keeps its tail.  All of it rests on "written before read".  The kernels on these
paths are free of float atomics (the one exception met, fi_error_map, is held to the oracle instead: BY_ATOMICS below), so the
same call after another history must give the same BITS; any difference is a read of something the call did not write.

A clean answer is made with the pool emptied and off and the remembered spectral bounds and iteration predictions off
(fi.memory_pool(0), FI_NO_POOL, FI_NO_LAMBDA_CACHE, FI_LOOK_ALWAYS) in a new context, twice, and the two must agree bit for
bit.  Then:

  A  within one context: its vectors poisoned with NaN (history_cases.poison), then the solve; and a problem of 20 000 points
     re-assembled with 1 500 others;
  B  across contexts: a predecessor of the same shape with other data, solved, poisoned and destroyed, its blocks in the pool;
  C  the same with a predecessor one to three points longer per axis (blocks of another size, a stale tail behind the request);
     runs only where B passes, so that a stale index has shown itself in range first;
  D  the caches on: a predecessor on the same lattice, weights, options and tolerance whose data need other iteration counts;
     the successor converges and agrees within the bounds of
     test_gpu_multilevel.py::test_solves_without_looks_at_the_stop_flag, and a second one repeats its bits;
  E  the mesh, tree and extraction units over a pool full of NaN blocks of every size from 1 KB to a few MB.

Integer state (indices, lists, keys) is never poisoned, it only goes stale from the same lattice shape: a read of it shows
as a wrong answer, not as an access outside a buffer.  Torch stays out of this process."""
import contextlib
import gc
import math
import os

import numpy as np
import pytest

import history_cases as H
from util import oracle_weights, sphere_points

pytestmark = pytest.mark.gpu

CLEAN = {"FI_NO_POOL": "1", "FI_NO_LAMBDA_CACHE": "1", "FI_LOOK_ALWAYS": "1"}
POOLED = {"FI_NO_POOL": None, "FI_NO_LAMBDA_CACHE": "1", "FI_LOOK_ALWAYS": "1"}
CACHED = {"FI_NO_POOL": None, "FI_NO_LAMBDA_CACHE": None, "FI_LOOK_ALWAYS": None}
SWITCHES = ("FI_NO_POOL", "FI_NO_LAMBDA_CACHE", "FI_LOOK_ALWAYS", "FI_LINEAR_START", "FI_SYNC_ALLOC_FILL", "FI_NO_TAIL")


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


@contextlib.contextmanager
def env(settings, case=None):
    """the switches of one arm (None: unset), the case's own on top; what was there before comes back"""
    want = {k: None for k in SWITCHES}
    want.update(settings)
    if case is not None:
        want.update(case.get("env", {}))
    was = {k: os.environ.get(k) for k in want}
    try:
        for k, v in want.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in was.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_same(got, want, what):
    """every entry of two answers (dicts, or sequences of arrays / None / numbers) bit for bit"""
    if isinstance(want, dict):
        assert set(got) == set(want), what
        for k in want:
            assert_same(got[k], want[k], "%s: %s" % (what, k))
    elif isinstance(want, (tuple, list)):
        assert len(got) == len(want), what
        for i, (a, b) in enumerate(zip(got, want)):
            assert_same(a, b, "%s[%d]" % (what, i))
    elif want is None:
        assert got is None, what
    elif isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, what
        if not np.array_equal(_bits(got), _bits(want)):
            raw = np.dtype("u%d" % got.itemsize)
            bad = np.flatnonzero(np.ascontiguousarray(got).reshape(-1).view(raw) != np.ascontiguousarray(want).reshape(-1).view(raw))
            nan = int(np.isnan(got).sum()) if got.dtype.kind == "f" else 0
            raise AssertionError("%s: %d of %d entries differ (first at %d: %r against %r), %d NaN" %
                                 (what, len(bad), got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]], nan))
    else:
        assert _bits(np.asarray(got)).tobytes() == _bits(np.asarray(want)).tobytes(), "%s: %r against %r" % (what, got, want)


# ---- the measuring stick ------------------------------------------------------------------------------------------------------

# The one path found NOT reproducible: fi_error_map.  k_error_rows (fi_operator.hip) adds every data row's blame to its 2^D
# lattice points with atomic_add, so where rows share a point the order of the additions, and with it the rounding, is the
# hardware's (two clean runs of the fp32 cases differ in the last bit of a few entries out of thousands).  Its output is held,
# clean and polluted alike, to the oracle's generate_error_map at the tolerance of
# test_gpu_solve.py::test_error_map_equals_reference_blame: 2e-4 of the largest entry (the oracle sums in fp32).
BY_ATOMICS = ("error_map",)
ERROR_MAP_TOL = 2e-4

_CLEAN = {}
_BLAME = {}


def bitwise(answer):
    return {k: v for k, v in answer.items() if k not in BY_ATOMICS}


def check_error_map(oracle, fi, case, answer, what, salt=0, n=None):
    if "error_map" not in answer:
        return
    key = (case["id"], salt, n)
    if key not in _BLAME:
        pos, _nrm, val = H.points(case, salt, n)
        w = H.weights(fi, case)
        fo = oracle.LatticeField(case["sizes"])
        fo.add_field_constraints(oracle_weights(oracle, w))
        fo.add_value_constraints(pos, val, w.data_pos)
        _BLAME[key] = np.asarray(fo.error_map(H.probe(case)), np.float64)
    want = _BLAME[key]
    got = answer["error_map"]
    assert got.dtype == np.float32 and got.shape == want.shape and not np.isnan(got).any(), what
    worst = np.abs(got - want).max() / np.abs(want).max()
    assert worst <= ERROR_MAP_TOL, "%s: error_map off the oracle's by %.2e of its largest entry" % (what, worst)


def clean_answer(fi, oracle, case, salt=0, n=None, switches=None):
    """The case's problem (points of seed `salt`) solved by a new context with nothing left over from anything: made twice,
    bit-equal, kept for every arm.  switches: further test switches for these runs (kept under their own key)."""
    key = (case["id"], salt, n, tuple(sorted((switches or {}).items())))
    if key not in _CLEAN:
        pts = H.points(case, salt, n)
        got = []
        with env(dict(CLEAN, **(switches or {})), case):
            for _ in range(2):
                assert fi.memory_pool(0) == 0
                f = H.make(fi, case, pts)
                got.append(H.answer(f, case))
                del f
                gc.collect()
                assert fi.memory_pool() == 0
        assert_same(bitwise(got[1]), bitwise(got[0]), "%s: two clean runs" % case["id"])
        for g in got:
            check_error_map(oracle, fi, case, g, "%s, clean" % case["id"], salt, n)
        if case.get("num_levels"):
            assert got[0]["num_levels"] == case["num_levels"], "the lattice does not give the levels the case is about"
        assert not np.isnan(got[0]["solution_f64"]).any()
        _CLEAN[key] = got[0]
    return _CLEAN[key]


@pytest.mark.parametrize("cid", H.TAIL_IDS)
def test_the_smallest_level_runs_in_the_one_workgroup_engine(fi, oracle, cid):
    """The case is there for its last level in the small-level engine (fi_tail.hip).  With FI_NO_TAIL the tiled kernels run that
    level: the same smoothers, constants and transfers in another order of sums, so -- as in
    test_gpu_multilevel.py::test_small_levels_in_one_workgroup_equal_the_tiled_kernels -- the iteration count within one and
    the solution within 3e-4 (an fp32 solve to 1e-5), but NOT the same bits.  Equal bits would mean that the engine had not
    run, and that no arm of this module reaches it."""
    case = H.BY_ID[cid]
    clean = clean_answer(fi, oracle, case)
    tiled = clean_answer(fi, oracle, case, switches={"FI_NO_TAIL": "1"})
    assert clean["converged"] == 1 and tiled["converged"] == 1
    assert abs(clean["iterations"] - tiled["iterations"]) <= 1
    scale = np.abs(tiled["solution_f64"]).max()
    assert np.abs(clean["solution_f64"] - tiled["solution_f64"]).max() <= 3e-4 * scale
    assert not np.array_equal(_bits(clean["solution_f64"]), _bits(tiled["solution_f64"])), "FI_NO_TAIL changes nothing"


# ---- A: within one context ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", H.IDS)
def test_a_poisoned_vectors_of_the_context_itself(fi, oracle, cid):
    from field_interpolation_amd._capi import FiError
    case = H.BY_ID[cid]
    clean = clean_answer(fi, oracle, case)
    with env(CLEAN, case):
        assert fi.memory_pool(0) == 0
        f = H.make(fi, case, H.points(case))
        f.assemble()
        H.poison(f, case, FiError)
        got = H.answer(f, case)
        assert not np.isnan(got["solution_f64"]).any()
        assert_same(bitwise(got), bitwise(clean), "%s after NaN in the context's own vectors" % cid)
        check_error_map(oracle, fi, case, got, cid)
        # ... and once more behind a whole solve and another poisoning (the kept vectors of a finished solve)
        H.poison(f, case, FiError)
        got = H.answer(f, case)
        assert_same(bitwise(got), bitwise(clean), "%s, second round" % cid)
        check_error_map(oracle, fi, case, got, cid)
        del f
        gc.collect()


@pytest.mark.parametrize("cid", H.SHRINK_IDS)
def test_a_fewer_points_on_the_same_context(fi, oracle, cid):
    """20 000 points, then 1 500 others on the same context: every data-dependent buffer shrinks and keeps its tail.  (Value
    rows under the default model weights: the polynomial's bound comes from the lattice and the model alone and no solve here
    widens it -- a widening would show as a breakdown-and-restart in the iteration counts, which are compared.)"""
    case = H.BY_ID[cid]
    clean = clean_answer(fi, oracle, case, salt=5, n=1500)
    with env(CLEAN, case):
        assert fi.memory_pool(0) == 0
        f = H.make(fi, case, H.points(case, salt=6, n=20000))
        big = H.answer(f, case)
        assert big["converged"] == 1 or big["iterations"] == case["max_it"]
        f.clear_points()
        H.add_data(fi, f, case, H.weights(fi, case), H.points(case, salt=5, n=1500))
        got = H.answer(f, case)
        assert_same(bitwise(got), bitwise(clean), "%s: 1 500 points behind 20 000 on one context" % cid)
        check_error_map(oracle, fi, case, got, cid, salt=5, n=1500)
        del f
        gc.collect()


# ---- B, C: across contexts ----------------------------------------------------------------------------------------------------

_ARM_B = {}


def _across(fi, oracle, case, pred_sizes, pred_pts, what):
    from field_interpolation_amd._capi import FiError
    clean = clean_answer(fi, oracle, case)
    with env(POOLED, case):
        assert fi.memory_pool(0) == 0
        try:
            pred = H.make(fi, case, pred_pts, sizes=pred_sizes, coo_salt=1)
            H.answer(pred, case)                   # (every buffer the successor will ask for exists, at its size)
            H.poison(pred, case, FiError)
            del pred
            gc.collect()
            held = fi.memory_pool()
            assert held > 0
            f = H.make(fi, case, H.points(case))
            got = H.answer(f, case)
            alive = fi.memory_pool()
            taken = (held - alive) / held
            assert alive < held, "%s: no pooled block was taken" % what
            assert_same(bitwise(got), bitwise(clean), "%s (%.0f %% of the pool taken)" % (what, 100 * taken))
            check_error_map(oracle, fi, case, got, what)
            del f
            gc.collect()
            after = fi.memory_pool()
            assert after <= 1.05 * held, "%s: the pool grew from %d to %d bytes (%.0f %% had been taken)" % (what, held, after, 100 * taken)
        finally:
            gc.collect()
            fi.memory_pool(0)


def _arm_b(fi, oracle, case):
    cid = case["id"]
    if cid not in _ARM_B:
        _ARM_B[cid] = "failed"
        # other points and other values, a seventh more of them: the predecessor's data-dependent blocks hold the successor's
        _across(fi, oracle, case, None, H.points(case, salt=3, n=case["n"] + case["n"] // 7 + 5), "%s after a predecessor of the same shape" % cid)
        _ARM_B[cid] = "passed"
    return _ARM_B[cid]


@pytest.mark.parametrize("cid", H.IDS)
def test_b_blocks_of_a_poisoned_predecessor_same_shape(fi, oracle, cid):
    assert _arm_b(fi, oracle, H.BY_ID[cid]) == "passed", "arm B has failed for this case earlier in this run"


@pytest.mark.parametrize("cid", H.IDS)
def test_c_blocks_of_a_larger_poisoned_predecessor(fi, oracle, cid):
    case = H.BY_ID[cid]
    assert _arm_b(fi, oracle, case) == "passed", "arm B fails for this case: the larger predecessor is not run"
    sizes = [s + 1 + (k + len(cid)) % 3 for k, s in enumerate(case["sizes"])]
    _across(fi, oracle, case, sizes, H.points(case), "%s after a predecessor of %s" % (cid, "x".join(map(str, sizes))))


# ---- D: remembered bounds and predictions -----------------------------------------------------------------------------------

# What the process remembers (fi_memory_pool(0) forgets it): the polynomial's spectral bound per (precision, lattice, model
# weights) -- LambdaKey, fi_poly.hip; every level of a hierarchy, the slabs' too -- and the iterations a solve took per
# (lattice, model, level, tolerance, kind of rows) -- PredKey, fi_cg.hip; undivided lattices only.  Arm D runs the cases on
# whose path one of them lies.  Cases 1, 2, 3, 10 and 11 are left out because neither does: no levels (no prediction), no
# polynomial (poly_terms <= 1, wide rows, triplet rows), so nothing remembered is ever looked up for them.
#   "a fifth of the points": the same keys throughout -- the bound AND the predictions reach the successor.
#   "the other kind of data": the issue's second predecessor.  PredKey holds whether the rows are value rows only, which comes
#   from the data, so this predecessor's predictions are filed under another key and never reach the successor: this leg
#   tests the remembered bound alone.
# Solution bound: test_solves_without_looks_at_the_stop_flag allows 3e-6 between two solves to a relative residual of 1e-8
# ("~1e-6 apiece"), i.e. 300 x the tolerance for the pair; the same amplification at the case's own tolerance: 300 x tol
# (3e-3 for the fp32 solves to 1e-5).  Case 7 stops by the field rule, which ignores the residual tolerance: there the
# rule's own contract takes the place of true_residual <= 1.01 tol -- stopped by the field test with an estimate within
# field_tol -- and each field is within twice field_tol of the converged one (the margin test_gpu_field_rule.py asserts
# against the oracle), so two of them within 4 x field_tol.
@pytest.mark.parametrize("kind", ["a fifth of the points", "the other kind of data"])
@pytest.mark.parametrize("cid", H.CACHE_IDS)
def test_d_remembered_bounds_and_predictions(fi, oracle, cid, kind):
    case = H.BY_ID[cid]
    clean = clean_answer(fi, oracle, case)
    assert clean["converged"] == 1 and clean["iterations"] < case["max_it"]
    tol = case["tol"]
    if kind == "a fifth of the points":
        pred_pts = H.points(case, salt=3, n=case["n"] // 5)
    else:
        pred_pts = H.points(case, salt=3, data="values" if case["data"] == "oriented" else "oriented")
    with env(CACHED, case):
        assert fi.memory_pool(0) == 0
        try:
            pred = H.make(fi, case, pred_pts)           # same lattice, weights, options and tolerance (the keys: see above)
            first = H.answer(pred, case)               # (it may run into max_it: what it leaves behind is what counts)
            del pred
            gc.collect()
            got = []
            for _ in range(2):
                f = H.make(fi, case, H.points(case))
                got.append(H.answer(f, case))
                del f
                gc.collect()
            a = got[0]
            scale = np.abs(clean["solution_f64"]).max()
            apart = np.abs(a["solution_f64"] - clean["solution_f64"]).max() / scale
            print("%s behind %s (%d iterations): %d iterations against %d clean, true residual %.3e, fields %.2e apart" %
                  (cid, kind, first["iterations"], a["iterations"], clean["iterations"], a["true_residual"], apart))
            assert a["converged"] == 1
            assert abs(a["iterations"] - clean["iterations"]) <= max(2, clean["iterations"] // 4)
            if case.get("field_tol"):
                assert a["field_rounds"] == 1 and 0.0 <= a["field_estimate"] <= case["field_tol"]
                assert apart <= 4.0 * case["field_tol"]
            else:
                assert a["true_residual"] <= 1.01 * tol
                assert apart <= 300.0 * tol
            assert_same(bitwise(got[1]), bitwise(got[0]), "%s: the second successor" % cid)
        finally:
            gc.collect()
            fi.memory_pool(0)


# ---- E: the geometry and mesh units over a polluted pool ---------------------------------------------------------------------

def _ladder(fi):
    """NaN-holding blocks of every size from about 1 KB to a few MB, a factor of at most 1.5 apart: 1-D and 2-D contexts in
    both precisions, each poisoned and destroyed.  -> bytes in the pool"""
    from field_interpolation_amd._capi import FiError
    w = fi.Weights(data_gradient=0.0)
    case = {"tol": 1e-5}
    nbytes, k = 1024.0, 0
    while nbytes < 5e6:
        dtype = "f32" if k % 2 == 0 else "f64"
        n = int(nbytes) // (4 if dtype == "f32" else 8)
        sizes = [n] if k % 4 < 2 else [max(8, int(math.sqrt(n))), max(8, n // max(8, int(math.sqrt(n))))]
        f = fi.LatticeField(sizes, dtype=dtype)
        f.add_field_constraints(w)
        pos = np.stack([np.linspace(1.0, s - 2.0, 5) for s in sizes], axis=1).astype(np.float32)
        f.add_points(1.0, w.value_kernel, 0.0, w.gradient_kernel, pos, None, None, values=np.ones(5, np.float32))
        f.assemble()
        H.poison(f, case, FiError)
        del f
        nbytes *= 1.45
        k += 1
    gc.collect()
    return fi.memory_pool()


def _strip_mesh(ndim, nv, npr):
    """the mesh of tests/test_gpu_mesh_scratch.py::mesh_case: a strip with chords, two loose primitives, one unused vertex"""
    rng = np.random.default_rng(1000 * ndim + 10 * nv + npr)
    used = nv - 1
    body = used - 2 * ndim
    prims = [list(range(i, i + ndim)) if i % 2 == 0 or ndim == 2 else [i + 1, i, i + 2] for i in range(body - ndim + 1)]
    prims += [list(range(body + ndim * k, body + ndim * (k + 1))) for k in range(2)]
    extra = npr - len(prims)
    assert 0 < extra < 10
    prims += [[0, 2 * k + 2, 2 * k + 4][:ndim] for k in range(extra)]
    idx = np.array(prims, np.int32)[rng.permutation(npr)]
    v = (rng.normal(size=(nv, ndim)) * 2.0).astype(np.float32)
    nrm = None
    if ndim == 3:
        nrm = rng.normal(size=(nv, 3))
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    return v, nrm, idx


def _smooth(sizes, seed):
    """a sphere's distance field with a ripple: a closed surface with a few thousand primitives"""
    grid = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sizes[::-1]], indexing="ij")[::-1]
    c = [(s - 1) / 2.0 for s in sizes]
    r = np.sqrt(sum((g - ci) ** 2 for g, ci in zip(grid, c))) - 0.3 * (min(sizes) - 1)
    rng = np.random.default_rng(seed)
    ripple = sum(np.sin(g * rng.uniform(0.3, 0.9) + rng.uniform(0, 6)) for g in grid)
    return (r + 0.4 * ripple).reshape(-1).astype(np.float32)


# a count pass of the extractors runs one work group per 256 lattice points (cells): 63, 64 and 64.5 groups
LATTICES = {2: ([126, 128], [128, 128], [129, 128]), 3: ([28, 24, 24], [32, 32, 16], [43, 24, 16])}
EDGE = (63, 64, 65)
CLOUD = 20000            # above one block of the sorts (1024 threads x 8 items) and above their 16 384-item threshold


class Meter:
    """the bytes the pool lost across the unit calls alone (the inputs of a group are made outside the spans)"""

    def __init__(self, fi):
        self.fi, self.taken = fi, {}

    @contextlib.contextmanager
    def __call__(self, unit):
        before = self.fi.memory_pool()
        yield
        self.taken[unit] = self.taken.get(unit, 0) + before - self.fi.memory_pool()


def _group_extraction(fi, meter):
    out = {}
    for ndim, shapes in LATTICES.items():
        for sizes in shapes:
            name = "x".join(map(str, sizes))
            f = np.random.default_rng(sum(sizes)).normal(size=int(np.prod(sizes))).astype(np.float32)
            big = [s + 1 for s in sizes]
            fb = np.random.default_rng(sum(big)).normal(size=int(np.prod(big))).astype(np.float32)
            rng = np.random.default_rng(ndim)
            pos = np.stack([rng.uniform(-1.5, s + 0.5, 1000) for s in sizes], axis=1).astype(np.float32)
            with meter("iso_surface"):
                out["iso " + name] = tuple(fi.iso_surface(f, sizes, 0.0))
            with meter("dual_contour"):
                out["dual " + name] = tuple(fi.dual_contour(fb, big, 0.0))
            with meter("sample"):
                for cubic in (False, True):
                    out["sample %s cubic=%d" % (name, cubic)] = tuple(fi.sample_field(f, sizes, pos, gradients=True, cubic=cubic))
                    out["sample values %s cubic=%d" % (name, cubic)] = fi.sample_field(f, sizes, pos[:65], cubic=cubic)
        sizes = shapes[2]
        g = _smooth(sizes, ndim)
        for method in ("iso", "dual"):
            with meter("redistance"):
                out["redistance %d-D %s" % (ndim, method)] = fi.redistance(g, sizes, 0.0, method=method)
    return out


def _group_points(fi, meter):
    out = {}
    for ndim, n in [(3, m) for m in EDGE + (CLOUD,)] + [(2, 65), (2, CLOUD)]:
        sizes = [20, 18, 16][:ndim]
        rng = np.random.default_rng(10 * n + ndim)
        pos, _ = sphere_points(rng, sizes, n, noise=0.2)
        q = np.stack([rng.uniform(-3.0, s + 2.0, 1000) for s in sizes], axis=1).astype(np.float32)
        name = "%d points in %d-D: " % (n, ndim)
        with meter("PointIndex"):
            index = fi.PointIndex(pos)
        with meter("nearest"):
            out[name + "nearest"] = tuple(index.nearest(q, indices=True))
        with meter("knn"):
            out[name + "knn"] = tuple(index.knn(q, 9))
        with meter("estimate_normals"):
            nrm, var = index.estimate_normals(k=8, variation=True)
        out[name + "estimate_normals"] = (nrm, var)
        with meter("orient_normals"):
            out[name + "orient_normals"] = tuple(index.orient_normals(nrm, k=8, components=True))
        with meter("distance_field"):
            out[name + "distance_field"] = tuple(index.distance_field(sizes, indices=True))
        del index
    return out


def _group_surface(fi, meter):
    out = {}
    meshes = [("strip %d-D %d/%d" % (ndim, nv, npr), _strip_mesh(ndim, nv, npr)[0], _strip_mesh(ndim, nv, npr)[2], [8, 8, 8][:ndim])
              for ndim in (3, 2) for nv, npr in ((63, 65), (64, 64), (65, 63))]
    for ndim, sizes in ((3, [24, 22, 20]), (2, [129, 128])):
        m = fi.iso_surface(_smooth(sizes, 7 + ndim), sizes, 0.0)
        meshes.append(("contour %d-D" % ndim, m.vertices, m.indices, sizes))
    for name, v, idx, sizes in meshes:
        ndim = v.shape[1]
        rng = np.random.default_rng(len(v))
        lo, hi = v.min(axis=0) - 1.0, v.max(axis=0) + 1.0
        q = rng.uniform(lo, hi, (1000, ndim)).astype(np.float32)
        d = rng.normal(size=(1000, ndim)).astype(np.float32)
        with meter("SurfaceIndex"):
            s = fi.SurfaceIndex(v, idx)
        with meter("distance"):
            out[name + ": distance"] = tuple(s.distance(q, primitives=True, closest=True))
        with meter("raycast"):
            out[name + ": raycast"] = tuple(s.raycast(q, d, bary=True))
        with meter("count_hits"):
            out[name + ": count_hits"] = s.count_hits(q, d)
        with meter("contains"):
            out[name + ": contains"] = s.contains(q)
        with meter("signed_distance_field"):
            out[name + ": signed_distance_field"] = tuple(s.signed_distance_field(sizes, primitives=True))
        del s
    return out


def _group_meshes(fi, meter):
    out = {}
    meshes = [("strip %d-D %d/%d" % (ndim, nv, npr),) + _strip_mesh(ndim, nv, npr) for ndim in (3, 2) for nv in EDGE for npr in EDGE]
    m = fi.iso_surface(_smooth([24, 22, 20], 3), [24, 22, 20], 0.0)
    meshes.append(("contour 3-D", m.vertices, m.normals, m.indices))
    for name, v, nrm, idx in meshes:
        mesh = fi.IsoMesh(v, nrm, idx, None)
        with meter("mesh_parts"):
            parts = fi.mesh_parts(mesh)
        out[name + ": mesh_parts"] = tuple(np.asarray(a) for a in parts)
        keep = np.arange(len(parts.size)) == 0
        with meter("select_parts"):
            out[name + ": select_parts"] = tuple(fi.select_parts(mesh, keep))
        for placement in ("quadric", "mean"):
            with meter("simplify_mesh"):
                simple, vmap = fi.simplify_mesh(mesh, 1.0, placement=placement, vertex_map=True)
            out[name + ": simplify_mesh " + placement] = tuple(simple) + (vmap,)
    return out


def _group_robust(fi, meter):
    """residuals per point and the reweighted solves: one workgroup's worth of points and a cloud beyond the sorts' threshold.
    The context is made, assembled and solved outside the spans."""
    out = {}
    for n in (65, CLOUD):
        sizes = [24, 20, 16]
        rng = np.random.default_rng(n)
        pos = np.stack([rng.uniform(0.0, s - 1.0, n) for s in sizes], axis=1).astype(np.float32)
        val = (np.linalg.norm(pos - 8.0, axis=1) - 5.0 + 0.05 * rng.normal(size=n)).astype(np.float32)
        val[::9] += 4.0                                                          # outliers
        w = fi.Weights(data_gradient=0.0)
        f = fi.LatticeField(sizes, dtype="f32")
        f.add_field_constraints(w)
        f.set_polynomial(4)
        f.add_points(w.data_pos, w.value_kernel, 0.0, w.gradient_kernel, pos, None, None, values=val)
        f.assemble()
        x, it, rel = f.solve_cg(None, 300, 1e-5)
        with meter("point_residuals"):
            out["robust %d: point_residuals" % n] = f.point_residuals()
        with meter("solve_robust"):
            field, omega, st = f.solve_robust(None, loss="huber", rounds=2, max_iterations=300, error_tolerance=1e-5)
        out["robust %d: solve_robust" % n] = (np.array(x, copy=True), field, omega, np.array([st["rounds"], st["iterations"], st["points_used"]]),
                                              np.float32(st["scale"]))
        out.setdefault("keep alive", []).append(f)      # (a context destroyed here would hand its blocks TO the pool)
    return out


GROUPS = {"extraction": _group_extraction, "points": _group_points, "surface": _group_surface, "meshes": _group_meshes,
          "robust": _group_robust}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_e_units_over_a_pool_of_poisoned_blocks(fi, group):
    call = GROUPS[group]
    clean = []
    with env(CLEAN):
        for _ in range(2):
            assert fi.memory_pool(0) == 0
            got = call(fi, Meter(fi))
            got.pop("keep alive", None)
            gc.collect()
            clean.append(got)
    assert_same(clean[1], clean[0], "%s: two clean runs" % group)
    with env(POOLED):
        assert fi.memory_pool(0) == 0
        try:
            held = _ladder(fi)
            assert held > 2e6
            meter = Meter(fi)
            got = call(fi, meter)
            alive = got.pop("keep alive", None)
            taken = sum(meter.taken.values())
            print("%s: bytes of the pool's %d taken by %s" % (group, held, meter.taken))
            assert taken > 0, "%s: its units took no pooled block (%s)" % (group, meter.taken)
            assert_same(got, clean[0], "%s over a polluted pool (%.1f %% of it taken by the units)" % (group, 100.0 * taken / held))
            del alive
        finally:
            gc.collect()
            fi.memory_pool(0)
