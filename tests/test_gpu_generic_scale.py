"""The generic-row path (fi_add_rows_coo / GradientKernel::kLinearInterpolation -> fi_generic.hip) beyond one sort block and
beyond one grid of its capped launches: >= 300 000 unknowns, >= 400 000 rows, >= 2 000 000 triplets, against the numpy
restatement of tests/generic_reference.py (itself checked on the CPU by tests/test_generic_reference.py).  Where the inputs
are small integers the device must give the reference's bits; where they are real numbers the bound is k * u * scale with k the
longest chain of additions on the path, u the precision's unit roundoff and scale the sum of the absolute terms."""
import functools

import numpy as np
import pytest

import generic_reference as gr
from test_gpu_generic import TOL, _check
from util import build_pair, random_points

pytestmark = pytest.mark.gpu

NP = {"f32": np.float32, "f64": np.float64}
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
N, M, NTRIP = 300_007, 400_003, 2_200_000          # unknowns, rows, triplets drawn (cases A, B, D, E, I)
EXACT = [(21, N, M, NTRIP, False), (22, N, M, NTRIP, True)]
NRUNS = 120_000                                     # case C: runs of 3 .. 40 duplicates, 2.6 M triplets
NSMOOTH = 300_007                                   # cases H, J


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _rows_only(fi, n, dtype, batches=()):
    f = fi.LatticeField([n], dtype=dtype)
    f.add_field_constraints(fi.Weights(model_2=0.0))            # no lattice model: the rows are everything
    for b in batches:
        f.add_rows_coo(*b)
    return f


@functools.lru_cache(maxsize=2)
def _exact(seed, n, m, ntrip, structures):
    batches, x, info = gr.exact_case(seed, n, m, ntrip, structures)
    R = gr.GenericRows(n, batches)
    assert R.exact_in_fp32(x) < 2 ** 24                          # before touching the device
    return batches, x, R


@functools.lru_cache(maxsize=1)
def _real():
    batches, x = gr.real_case(31, N, M, NTRIP)
    return batches, x, gr.GenericRows(N, batches)


def _assert_exact(f, R, x, T):
    np.testing.assert_array_equal(f.Atb(), R.Atb(T))
    np.testing.assert_array_equal(f.diag(), R.diag(T))
    y = f.apply_AtA(x)
    np.testing.assert_array_equal(y, R.apply(x, T))
    np.testing.assert_array_equal(y, f.apply_AtA(x))           # no atomics: the same bits again
    return y


# ---- A, B -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("seed,n,m,ntrip,structures", EXACT)
def test_exact_at_scale(fi, dtype, seed, n, m, ntrip, structures):
    """Values in {+-1, 0}, rhs and x in {-1, 0, 1}, three batches of unequal size, the triplets in a random permutation:
    every intermediate is an integer below 2**24 (exact_in_fp32), so A^T b, diag and A^T A x equal the reference's to the bit
    in both precisions whatever the order of the additions -- a dropped, doubled, misplaced or mis-merged triplet changes
    an integer.  With `structures` (generic_reference.exact_case): a row and a column of 50 000 entries, 20 000 empty rows
    with rhs, untouched unknowns, explicit zeros, all-zero rows, pairs repeated 10 000 times summing to 0 and to 400."""
    batches, x, R = _exact(seed, n, m, ntrip, structures)
    f = _rows_only(fi, n, dtype, batches)
    _assert_exact(f, R, x, NP[dtype])
    st = f.stats()
    assert st["num_generic_rows"] == R.m


# ---- I ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_device_memory_input_equals_host_memory_input(fi, dtype, _device_input):
    """fi_add_rows_coo with FI_DEVICE buffers (torch tensors on the GPU): the results of case B, bit for bit."""
    seed, n, m, ntrip, structures = EXACT[1]
    batches, x, R = _exact(seed, n, m, ntrip, structures)
    o, T = _device_input, NP[dtype]
    assert o["mixed_refused_" + dtype][0] and o["rows_" + dtype][0] == R.m
    np.testing.assert_array_equal(o["atb_" + dtype], R.Atb(T))
    np.testing.assert_array_equal(o["diag_" + dtype], R.diag(T))
    np.testing.assert_array_equal(o["y_" + dtype], R.apply(x, T))
    np.testing.assert_array_equal(o["y_" + dtype], o["y2_" + dtype])
    host = _rows_only(fi, n, dtype, batches)
    np.testing.assert_array_equal(o["atb_" + dtype], host.Atb())
    np.testing.assert_array_equal(o["diag_" + dtype], host.diag())
    np.testing.assert_array_equal(o["y_" + dtype], host.apply_AtA(x))


@pytest.fixture(scope="module")
def _device_input(tmp_path_factory):
    """Case B through tests/generic_torch_worker.py, a fresh process: torch must stay out of this one."""
    import os
    import subprocess
    import sys
    seed, n, m, ntrip, structures = EXACT[1]
    batches, x, R = _exact(seed, n, m, ntrip, structures)
    tmp = tmp_path_factory.mktemp("generic_device")
    arrays = {"n": np.array(n), "nbatches": np.array(len(batches)), "x": x}
    for k, (r, c, v, b) in enumerate(batches):
        arrays.update({"r%d" % k: r.astype(np.int32), "c%d" % k: c.astype(np.int32), "v%d" % k: v, "b%d" % k: b})
    np.savez(tmp / "in.npz", **arrays)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "generic_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp / "in.npz"), str(tmp / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(np.load(tmp / "out.npz"))


# ---- C ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_duplicates_are_summed_in_input_order(fi, dtype):
    """120 000 runs of 3 to 40 duplicates, run r on (row r, column r) with rhs 1, terms of the size of 2**24 (f32) or 2**53
    (f64) mixed with units, shuffled across runs with every run's own order kept: (A^T b)[r] is the folded value, and it
    must be the left-to-right sum in the context's precision bit for bit -- Eigen's setFromTriplets after a stable sort
    (DESIGN.md 1, 3).  A fold that combines partial sums, a + (b + c), or an unstable sort changes these bits
    (tests/test_generic_reference.py::test_order_case_is_order_sensitive)."""
    T = NP[dtype]
    batch, lengths = gr.order_case(12, NRUNS, T)
    R = gr.GenericRows(NRUNS, batch)
    want = R.fold(T)[2].astype(np.float64)
    f = _rows_only(fi, NRUNS, dtype, [batch])
    got = f.Atb()
    wrong = np.flatnonzero(got != want)
    print("%s: %d of %d runs differ from the left-to-right fold" % (dtype, len(wrong), NRUNS))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(f.diag(), (want * want).astype(T).astype(np.float64))


# ---- D ----------------------------------------------------------------------------------------------------------------
def _chain(R):
    run, row, col = R.chain_lengths()
    return run + row + col + 4


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_real_valued_at_scale(fi, dtype):
    """Normal values, 5 % duplicated (row, col), short rows and columns, three batches.  Every component within
    k * u * scale of the reference's fp64 result: k = longest duplicate run + longest row + longest column + 4 (input and
    output roundings and the two products) = 5 + 21 + 23 + 4 = 53 for this draw, computed from the input below; u = 2**-24
    or 2**-53; scale = |A|^T |A| |x| for the product, sum |a b| for A^T b, sum a^2 for the diagonal, with |A| summed over
    the duplicates' absolute values (generic_reference.abs_apply)."""
    batches, x, R = _real()
    k = _chain(R)
    assert k == 53
    f = _rows_only(fi, N, dtype, batches)
    tol = k * U[dtype]
    for name, got, want, scale in [("Atb", f.Atb(), R.Atb(), R.abs_Atb()), ("diag", f.diag(), R.diag(), R.abs_diag()),
                                   ("AtA x", f.apply_AtA(x), R.apply(x), R.abs_apply(x))]:
        ratio = np.abs(got - want) / np.maximum(tol * scale, 1e-300)
        print("%s %s: worst error / bound = %.3g" % (dtype, name, ratio.max()))
        assert np.all(np.abs(got - want) <= tol * scale), name
    np.testing.assert_array_equal(f.apply_AtA(x), f.apply_AtA(x))


# ---- E ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_error_map_at_scale(fi, dtype):
    """generate_error_map over D's 2.2 M raw triplets (duplicates not summed, grids of the capped launches strided
    twice over).  The kernels add with atomics, so the bound is not bitwise: (longest row + longest column + 2) * u * scale,
    scale = the map itself plus 2 |res| (|rhs| + sum |a x|) per blamed residual (generic_reference.abs_error_map), plus the
    fp32 rounding of the output array (fi_error_map returns float)."""
    batches, x, R = _real()
    _, row, col = R.chain_lengths()
    f = _rows_only(fi, N, dtype, batches)
    sol = x.astype(np.float32)
    got = f.error_map(sol).astype(np.float64)
    want = R.error_map(sol)
    bound = (row + col + 2) * U[dtype] * R.abs_error_map(sol) + 2.0 ** -24 * want
    print("%s error map: worst error / bound = %.3g" % (dtype, (np.abs(got - want) / np.maximum(bound, 1e-300)).max()))
    assert np.all(np.abs(got - want) <= bound)


def _tile_rows(sizes, ts, cross, seed):
    """A data row per unknown (weight 1, random target) and 2 short rows per unknown coupling it to random unknowns of its
    own tile -- or, with `cross`, to its lattice neighbours, whichever tile they lie in."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(sizes))
    i = np.arange(n, dtype=np.int64)
    ix, iy = i % sizes[0], i // sizes[0]
    rows, cols, vals = [i], [i], [np.ones(n, np.float32)]
    for k in range(2):
        if cross:
            jx, jy = (ix + 1) % sizes[0] if k == 0 else ix, iy if k == 0 else (iy + 1) % sizes[1]
        else:
            jx = (ix // ts) * ts + rng.integers(0, ts, n)
            jy = (iy // ts) * ts + rng.integers(0, ts, n)
        j = jy * sizes[0] + jx
        w = rng.uniform(0.2, 0.6, n).astype(np.float32)
        rows += [n + k * n + i, n + k * n + i]
        cols += [i, j]
        vals += [w, -w]
    rhs = np.r_[rng.normal(size=n), np.zeros(2 * n)].astype(np.float32)
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), rhs


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("cross", [False, True])
def test_tile_pass_at_scale(fi, dtype, cross):
    """k_generic_tile on a [640, 480] lattice (307 200 unknowns, 921 600 rows of at most 2 entries, tiles of 16).  Rows that
    never cross a tile: the tile operator is the whole of A^T A, so tile_pass(g) is the solution of
    (A^T A + 1e-6) x = A^T b whatever the guess.  Rows that do cross: the dense re-derivation of
    test_gpu_generic.py::test_tile_pass_on_materialised_rows (couplings to other tiles moved to the rhs twice) on a sample
    of 40 tiles.  Its tolerances (1e-6 / 5e-3 of the largest value)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    sizes, ts = [640, 480], 16
    n = sizes[0] * sizes[1]
    rows, cols, vals, rhs = _tile_rows(sizes, ts, cross, 5)
    R = gr.GenericRows(n, (rows, cols, vals, rhs))
    r, c, a = R.fold(np.float64)
    A = sp.csr_matrix((a, (r, c)), shape=(R.m, n))
    Mfull = (A.T @ A).tocsr()
    atb = R.Atb()
    g = np.random.default_rng(6).normal(size=n).astype(np.float32)
    tile = gr.tile_index(sizes, ts)
    if not cross:
        np.testing.assert_allclose(R.tile_apply(g, sizes, ts), R.apply(g), rtol=0, atol=1e-12 * R.abs_apply(g).max())
    f = fi.LatticeField(sizes, dtype=dtype)
    f.add_field_constraints(fi.Weights(model_2=0.0))
    f.add_rows_coo(rows, cols, vals, rhs)
    x = f.tile_pass(g, ts).astype(np.float64)
    tol = 1e-6 if dtype == "f64" else 5e-3
    if not cross:
        expect = spl.spsolve((Mfull + 1e-6 * sp.identity(n)).tocsc(), atb)
        assert np.abs(x - expect).max() <= tol * np.abs(expect).max()
        return
    g64 = g.astype(np.float64)
    sample = np.random.default_rng(7).choice(int(tile.max()) + 1, 40, replace=False)
    sample[:2] = [0, int(tile.max())]
    worst = 0.0
    for t in sample:
        mine = np.flatnonzero(tile == t)
        Mrows = Mfull[mine]
        Mtt = Mrows[:, mine].toarray()
        other = Mrows @ g64 - Mtt @ g64[mine]                              # M[mine, other] @ g[other]
        expect = np.linalg.solve(Mtt + 1e-6 * np.eye(len(mine)), atb[mine] - 2.0 * other)
        worst = max(worst, np.abs(x[mine] - expect).max() / np.abs(expect).max())
    print("%s tile pass, crossing rows: worst relative error over 40 tiles %.3g" % (dtype, worst))
    assert worst <= tol


# ---- F ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("sizes", [[96, 80, 72], [1024, 768]])
def test_generic_rows_on_top_of_a_lattice_at_scale(oracle, fi, dtype, sizes):
    """A lattice with model_2 and 50 000 oriented points (3-D: the marching kernel; 2-D: the tile kernel) plus 420 000
    wrap-around rows [-w at p near the far face of an axis, +w at q near its near face, same other coordinates] with
    targets, in two batches.  Product, A^T b and
    diag against the oracle's lattice part plus the reference's generic part: test_gpu_generic.py's TOL on the lattice
    part plus D's k * u * scale on the generic part."""
    rng = np.random.default_rng(len(sizes) + 40)
    n = int(np.prod(sizes))
    pos, nrm, pw, _ = random_points(rng, sizes, 50_000, margin=1.2)
    fo, fg = build_pair(oracle, fi, sizes, fi.Weights(), pos, nrm, pw, dtype=dtype)
    m = 420_000
    p0 = rng.integers(0, n, m)
    d = rng.integers(0, len(sizes), m)
    size_d, stride_d = np.array(sizes)[d], np.cumprod([1] + sizes[:-1])[d]
    coord = (p0 // stride_d) % size_d
    p = p0 + (size_d - 1 - rng.integers(0, 3, m) - coord) * stride_d      # within 3 planes of the far face of axis d ...
    q = p0 + (rng.integers(0, 3, m) - coord) * stride_d                   # ... tied to the near face: around the torus
    w = rng.uniform(0.2, 1.0, m).astype(np.float32)
    rows = np.repeat(np.arange(m, dtype=np.int64), 2)
    cols = np.stack([p, q], 1).ravel()
    vals = np.stack([-w, w], 1).ravel()
    rhs = rng.normal(scale=0.3, size=m).astype(np.float32)
    assert np.all(p - q >= (size_d - 6) * stride_d) and p.max() < n and q.min() >= 0
    batches = gr.split_batches(rows, cols, vals, rhs, [0, m // 3, m])
    for b in batches:
        fg.add_rows_coo(*b)
    R = gr.GenericRows(n, batches)
    AtA, atb, diag = fo.normal_equations()
    ku = _chain(R) * U[dtype]
    x = rng.normal(size=n).astype(np.float32).astype(np.float64)
    for name, got, want, bound in [
            ("Atb", fg.Atb(), atb + R.Atb(), TOL[dtype] * np.abs(atb).max() + ku * R.abs_Atb()),
            ("diag", fg.diag(), diag + R.diag(), TOL[dtype] * np.abs(diag).max() + ku * R.abs_diag()),
            ("AtA x", fg.apply_AtA(x), AtA @ x + R.apply(x), TOL[dtype] * (abs(AtA) @ np.abs(x)).max() + ku * R.abs_apply(x))]:
        print("%s %s %s: worst error / bound = %.3g" % (dtype, sizes, name, (np.abs(got - want) / bound).max()))
        assert np.all(np.abs(got - want) <= bound), name
    np.testing.assert_array_equal(fg.apply_AtA(x), fg.apply_AtA(x))


# ---- G ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_gradient_linear_interpolation_kernel_at_scale(oracle, fi, dtype):
    """GradientKernel::kLinearInterpolation on [64, 64, 64] with 100 000 points: 300 000 rows, 4.8 M triplets, 586 sort
    blocks.  Undivided and over 3 slabs against the oracle's explicit normal equations (test_gpu_generic.py's _check and
    TOL); the slabs' error map equals the undivided one to 1e-4."""
    sizes = [64, 64, 64]
    rng = np.random.default_rng(50)
    pos, nrm, pw, _ = random_points(rng, sizes, 100_000, margin=1.2)
    w = fi.Weights(data_gradient=0.9, gradient_kernel=fi.GradientKernel.kLinearInterpolation)
    fo, one = build_pair(oracle, fi, sizes, w, pos, nrm, pw, dtype=dtype)
    _check(fo, one, dtype)
    assert one.stats()["num_generic_rows"] == 300_000
    grp = fi.LatticeGroup(sizes, 3, dtype=dtype)
    grp.add_field_constraints(w)
    grp.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, pw)
    grp.assemble()
    AtA, atb, diag = fo.normal_equations()
    tol = TOL[dtype]
    assert np.abs(grp.Atb() - atb).max() <= tol * np.abs(atb).max()
    assert np.abs(grp.diag() - diag).max() <= tol * np.abs(diag).max()
    x = rng.normal(size=fo.num_unknowns)
    y = grp.apply_AtA(x)
    assert np.abs(y - AtA @ x).max() <= tol * (abs(AtA) @ np.abs(x)).max()
    np.testing.assert_array_equal(y, grp.apply_AtA(x))
    sol = rng.normal(size=fo.num_unknowns).astype(np.float32)
    e1, eg = one.error_map(sol), grp.error_map(sol)
    assert np.abs(eg - e1).max() <= 1e-4 * np.abs(e1).max()


# ---- H ----------------------------------------------------------------------------------------------------------------
def _smooth():
    import scipy.sparse as sp
    batches = gr.smooth_case(60, NSMOOTH)
    R = gr.GenericRows(NSMOOTH, batches)
    r, c, a = R.fold(np.float64)
    A = sp.csr_matrix((a, (r, c)), shape=(R.m, NSMOOTH))
    AtA = (A.T @ A).tocsr()
    d = AtA.diagonal()
    off = np.asarray(abs(AtA).sum(1)).ravel() - np.abs(d)
    assert (d - off).min() > 0
    kappa = (d + off).max() / (d - off).min()                    # Gershgorin: every eigenvalue lies in [min(d - off), max(d + off)]
    return batches, R, AtA, kappa


def test_fp64_solve_at_scale(fi):
    """One unit data row per unknown plus second differences of weight 0.25 on 300 007 unknowns: A^T A = I + D^T D / 16,
    Gershgorin bound kappa_G = 2 / 0.75.  solve_sparse_linear_exact: the residual recomputed by the reference from
    solution_f64() is <= 1e-11 (test_fp64_cg_matches_direct_solution's figure) and the error against scipy's direct
    solution of the reference's matrix is <= kappa_G * that residual."""
    import scipy.sparse.linalg as spl
    batches, R, AtA, kappa = _smooth()
    assert kappa <= 2.0 / 0.75 * (1 + 1e-6)
    f = _rows_only(fi, NSMOOTH, "f64", batches)
    assert fi.solve_sparse_linear_exact(f) is not None
    x = f.solution_f64()
    atb = R.Atb()
    res = np.linalg.norm(atb - R.apply(x)) / np.linalg.norm(atb)
    xs = spl.spsolve(AtA.tocsc(), atb)
    err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    print("fp64 solve: residual %.3g, error %.3g, kappa_G %.4g" % (res, err, kappa))
    assert res <= 1e-11
    assert err <= kappa * res


def test_fp32_solve_at_scale(fi):
    """The same system in fp32: solve_cg(None, 0, 1e-5); the residual recomputed by the reference from the returned field
    is <= 3e-5 (test_fp32_cg_reaches_reference_stop_rule's margin)."""
    batches, R, AtA, kappa = _smooth()
    f = _rows_only(fi, NSMOOTH, "f32", batches)
    x, it, rel = f.solve_cg(None, 0, 1e-5)
    atb = R.Atb()
    res = np.linalg.norm(atb - R.apply(x.astype(np.float64))) / np.linalg.norm(atb)
    print("fp32 solve: %d iterations, reported %.3g, recomputed %.3g" % (it, rel, res))
    assert rel <= 1e-5
    assert res <= 3 * 1e-5


# ---- J ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_lifecycle_at_scale(fi, dtype):
    """assemble() twice; clear_points and fresh rows; a fourth batch after a solve; refused batches -- on 300 007 unknowns
    and 600 000 rows in four batches.  The assembly is deterministic (stable sort, no floating-point atomics), so equal
    inputs give equal bits."""
    from field_interpolation_amd._capi import FiError
    two = gr.smooth_case(61, NSMOOTH)
    four = []
    for r, c, v, b in two:                                       # each of the two batches cut at a third of its rows
        four += gr.split_batches(r, c, v, b, [0, len(b) // 3, len(b)])
    x = np.random.default_rng(62).normal(size=NSMOOTH).astype(np.float32).astype(np.float64)

    def state(f):
        return f.Atb(), f.diag(), f.apply_AtA(x)

    def same(a, b):
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)

    whole = _rows_only(fi, NSMOOTH, dtype, four)
    want = state(whole)
    R = gr.GenericRows(NSMOOTH, four)
    k = _chain(R) * U[dtype]
    assert np.all(np.abs(want[0] - R.Atb()) <= k * R.abs_Atb()) and np.all(np.abs(want[2] - R.apply(x)) <= k * R.abs_apply(x))
    whole.assemble()
    same(state(whole), want)                                    # assemble() twice
    f = _rows_only(fi, NSMOOTH, dtype, four[:3])
    three = state(f)
    assert not np.array_equal(three[1], want[1])                # (the fourth batch's targets are 0: A^T b does not see it)
    assert f.solve_cg(None, 0, 1e-4) is not None
    f.add_rows_coo(*four[3])                                    # a fourth batch after a solve
    f.assemble()
    same(state(f), want)
    n3 = sum(len(b[3]) for b in four)
    for bad_r, bad_c in [(0, NSMOOTH), (len(four[0][3]), 0), (0, -1), (-1, 0)]:
        r, c, v, b = (a.copy() for a in four[0])
        r[len(r) // 2], c[len(c) // 2] = bad_r, bad_c           # one bad index in the middle of 100 000 good triplets
        with pytest.raises(FiError):
            f.add_rows_coo(r, c, v, b)
    assert f.stats()["num_generic_rows"] == n3
    f.assemble()
    same(state(f), want)                                        # the refused batches left nothing behind
    f.clear_points()
    for b in four[:3]:
        f.add_rows_coo(*b)
    same(state(f), three)                                       # clear_points + fresh rows: the fresh answer
