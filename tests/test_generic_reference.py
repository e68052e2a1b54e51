"""The numpy restatement of the generic-row path (tests/generic_reference.py) against independent implementations on the
CPU: scipy's COO -> CSR products, the oracle's normal equations and error map; and the properties the GPU cases of
tests/test_gpu_generic_scale.py rely on -- that their inputs are exact in fp32 where they claim it, and order-sensitive where
they claim that."""
import numpy as np
import pytest
import scipy.sparse as sp

import generic_reference as gr
from test_gpu_generic import _line_2d_like

EPS = 2.0 ** -53


@pytest.mark.parametrize("seed,n,m,ntrip", [(0, 50, 70, 400), (1, 3000, 2500, 40000), (2, 1, 5, 30)])
def test_reference_equals_scipy_products(seed, n, m, ntrip):
    """Random real values, many duplicates (the draws collide), three batches: A^T b, diag and A^T A x against scipy's
    tocsr() (which sums duplicates) at fp64 rounding: (terms added + 4) * 2**-53 * the sum of the absolute terms."""
    batches, x = gr.real_case(seed, n, m, ntrip, dup=0.3)
    R = gr.GenericRows(n, batches)
    A = sp.coo_matrix((R.vals.astype(np.float64), (R.rows, R.cols)), shape=(m, n)).tocsr()
    b = R.rhs.astype(np.float64)
    run, row, col = R.chain_lengths()
    k = run + row + col + 4
    assert np.all(np.abs(R.Atb() - A.T @ b) <= k * EPS * R.abs_Atb() + 1e-300)
    assert np.all(np.abs(R.diag() - np.asarray(A.multiply(A).sum(0)).ravel()) <= k * EPS * R.abs_diag() + 1e-300)
    assert np.all(np.abs(R.apply(x) - A.T @ (A @ x)) <= k * EPS * R.abs_apply(x) + 1e-300)
    r, c, v = R.fold(np.float64)
    assert len(v) == A.nnz and np.all(np.diff(r * n + c) > 0)
    # the float32 fold is the float64 fold to float32 rounding per addition
    v32 = R.fold(np.float32)[2]
    o, s, l = R.runs()
    scale = np.add.reduceat(np.abs(R.vals[o].astype(np.float64)), s)
    assert np.all(np.abs(v32 - v) <= l * 2.0 ** -24 * scale)


def test_fold_is_left_to_right():
    """[1, 1, 2**24] is 16 777 218 left to right and 16 777 216 as 1 + (1 + 2**24); batches restart their row numbers."""
    one = np.float32(1)
    vals = np.array([1, 1, 2 ** 24, 2 ** 24, 1, 1, 5], np.float32)
    rows, cols = np.array([0, 0, 0, 1, 1, 1, 0]), np.array([2, 2, 2, 2, 2, 2, 0])
    R = gr.GenericRows(3, [(rows, cols, vals, np.ones(2, np.float32)), (rows, cols, vals, np.ones(2, np.float32))])
    r, c, v = R.fold(np.float32)
    assert r.tolist() == [0, 0, 1, 2, 2, 3] and c.tolist() == [0, 2, 2, 0, 2, 2]
    assert v.tolist() == [5.0, 16777218.0, 16777216.0, 5.0, 16777218.0, 16777216.0]
    assert one + (one + np.float32(2 ** 24)) == np.float32(2 ** 24)
    assert R.fold(np.float64)[2].tolist() == [5.0, 16777218.0, 16777218.0] * 2


@pytest.mark.parametrize("n", [60, 300])
def test_reference_equals_oracle_on_line_2d_rows(oracle, n):
    """The hand-built rows of test_gpu_generic.py (data rows, second differences, a duplicated entry): normal equations
    and error map against the oracle library's."""
    fo = _line_2d_like(oracle, n=n)
    rows, cols, vals, rhs = fo.get()
    half = len(rhs) // 2
    first = rows < half
    R = gr.GenericRows(fo.num_unknowns, [(rows[first], cols[first], vals[first], rhs[:half]),
                                         (rows[~first] - half, cols[~first], vals[~first], rhs[half:])])
    AtA, atb, diag = fo.normal_equations()
    assert np.abs(R.Atb() - atb).max() <= 16 * EPS * R.abs_Atb().max()
    assert np.abs(R.diag() - diag).max() <= 16 * EPS * R.abs_diag().max()
    x = np.random.default_rng(n).normal(size=fo.num_unknowns)
    assert np.abs(R.apply(x) - AtA @ x).max() <= 16 * EPS * R.abs_apply(x).max()
    sol = x.astype(np.float32)
    ref = gr.GenericRows(fo.num_unknowns, (rows, cols, vals, rhs)).error_map(sol)
    got = fo.error_map(sol)                                     # float32 arithmetic, rows of at most 3 entries
    assert np.abs(got - ref).max() <= 16 * 2.0 ** -24 * R.abs_error_map(sol).max()


def test_error_map_does_not_sum_duplicates():
    """(row 0, col 1) twice with 1 and -1: summed, the row would blame column 0 alone; per triplet, column 1 gets 2/3."""
    R = gr.GenericRows(2, (np.array([0, 0, 0]), np.array([0, 1, 1]), np.array([1, 1, -1], np.float32), np.array([3], np.float32)))
    x = np.array([1.0, 5.0])
    np.testing.assert_allclose(R.error_map(x), [4.0 / 3.0, 8.0 / 3.0], rtol=1e-15)


@pytest.mark.parametrize("sizes,ts", [([10, 7], 4), ([5, 4, 3], 2), ([33], 8)])
def test_tile_apply_equals_masked_dense_product(sizes, ts):
    rng = np.random.default_rng(ts)
    n = int(np.prod(sizes))
    batches, x = gr.real_case(ts, n, 2 * n, 8 * n, dup=0.1)
    R = gr.GenericRows(n, batches)
    A = sp.coo_matrix((R.vals.astype(np.float64), (R.rows, R.cols)), shape=(R.m, n)).toarray()
    coords = np.stack(np.unravel_index(np.arange(n), sizes[::-1])[::-1], 1)
    tile = np.zeros(n, np.int64)
    for d in range(len(sizes) - 1, -1, -1):
        tile = tile * 64 + coords[:, d] // ts
    M = (A.T @ A) * (tile[:, None] == tile[None, :])
    got = R.tile_apply(x, sizes, ts)
    assert np.abs(got - M @ x).max() <= 64 * EPS * (np.abs(A).T @ (np.abs(A) @ np.abs(x))).max()
    assert np.array_equal(gr.tile_index(sizes, ts) == gr.tile_index(sizes, ts)[0], tile == tile[0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_order_case_is_order_sensitive(dtype):
    """Case C's generator: the left-to-right fold of a run differs from the fold a reduction by key performs when the run
    straddles two of its partial sums -- prefix + (suffix folded on its own) -- for some split point, in at least nine runs of ten
    (later terms of twice the size can round the difference away); from the right-to-left fold in most; the runs start at every offset modulo the sort's 8 192-pair block."""
    nruns = 120_000
    batch, lengths = gr.order_case(12, nruns, dtype)
    R = gr.GenericRows(nruns, batch)
    order, start, length = R.runs()
    assert np.array_equal(length, lengths) and lengths.min() >= 3 and lengths.max() <= 40 and len(R.vals) >= 2_000_000
    assert len(np.unique(start % 8192)) == 8192
    v = R.vals[order].astype(dtype)
    l2r = R.fold(dtype)[2]
    assert np.all(np.isfinite(l2r))
    # the shuffle kept each run's order: the stable sort gives back the generator's sequence
    _, v0 = gr.order_sensitive_runs(np.random.default_rng(12), nruns, dtype)
    assert np.array_equal(R.vals[order], v0)
    r2l = gr.fold_runs(v[::-1].copy(), len(v) - start - length, length, dtype)
    assert np.mean(l2r != r2l) >= 0.5
    differs = np.zeros(nruns, bool)
    for s in range(1, 40):                                       # prefix of s terms + the rest folded separately
        sel = np.flatnonzero(length > s)
        head = gr.fold_runs(v, start[sel], np.full(len(sel), s), dtype)
        tail = gr.fold_runs(v, start[sel] + s, length[sel] - s, dtype)
        differs[sel] |= (head + tail).astype(dtype) != l2r[sel]
    assert differs.mean() >= 0.9
    # the opening terms alone: (1 + 1) + 2**p against 1 + (1 + 2**p)
    p = dtype(2.0) ** (24 if dtype is np.float32 else 53)
    assert (dtype(1) + dtype(1)) + p == p + dtype(2) and dtype(1) + (dtype(1) + p) == p


EXACT = [(21, 300_007, 400_003, 2_200_000, False), (22, 300_007, 400_003, 2_200_000, True)]


@pytest.mark.parametrize("seed,n,m,ntrip,structures", EXACT)
def test_exact_cases_are_exact_in_fp32(seed, n, m, ntrip, structures):
    batches, x, info = gr.exact_case(seed, n, m, ntrip, structures)
    R = gr.GenericRows(n, batches)
    assert len(batches) == 3 and len({len(b[3]) for b in batches}) == 3
    assert R.n >= 300_000 and R.m >= 400_000 and len(R.vals) >= 2_000_000
    assert R.exact_in_fp32(x) < 2 ** 24
    # float32 and float64 folds agree to the bit: nothing was rounded
    assert np.array_equal(R.fold(np.float32)[2].astype(np.float64), R.fold(np.float64)[2])
    if structures:
        run, row, col = R.chain_lengths()
        assert run == 10_000 and row == 50_000 and col >= 50_000
        r, c, v = R.fold(np.float32)
        assert v[(r == info["zero_sum"][0]) & (c == info["zero_sum"][1])].tolist() == [0.0]
        assert v[(r == info["sum_400"][0]) & (c == info["sum_400"][1])].tolist() == [400.0]
        counts = np.bincount(R.rows, minlength=R.m)
        assert len(info["empty_rows"]) == 20_000 and not counts[info["empty_rows"]].any() and np.all(R.rhs[info["empty_rows"]] != 0)
        edges = np.cumsum([0] + [len(b[3]) for b in batches])
        assert set(np.r_[edges[:-1], edges[1:] - 1]) <= set(info["empty_rows"].tolist())
        assert not np.isin(R.cols, info["dead_cols"]).any() and {0, n - 1} <= set(info["dead_cols"].tolist())
        assert (R.vals == 0).sum() >= 10_000
        assert counts[info["zero_rows"]].min() >= 1 and not R.vals[np.isin(R.rows, info["zero_rows"])].any()
        assert np.bincount(R.cols, minlength=n)[info["long_col"]] >= 50_000
        others = R.rows[R.cols == info["long_col"]]
        assert counts[others[others != info["long_row"]]].max() <= 40           # the long column's other rows are short
        # the repeated pairs' copies lie all over their batch
        where = np.flatnonzero((R.rows == info["sum_400"][0]) & (R.cols == info["sum_400"][1]))
        assert len(where) == 10_000 and where.max() - where.min() > 500_000


def test_exact_in_fp32_rejects_what_is_not_exact():
    rows, cols, rhs = np.array([0, 0, 1]), np.array([0, 0, 1]), np.ones(2, np.float32)
    ok = gr.GenericRows(2, (rows, cols, np.array([3, -2, 4], np.float32), rhs))
    assert ok.exact_in_fp32() == 16.0                                         # diag: 4 * 4
    big = gr.GenericRows(2, (rows, cols, np.array([2 ** 23, 2 ** 23, 1], np.float32), rhs))
    assert big.exact_in_fp32() >= 2 ** 24                                     # the fold itself reaches 2**24
    sq = gr.GenericRows(2, (rows, cols, np.array([1, 1, 5000], np.float32), rhs))
    assert sq.exact_in_fp32() >= 2 ** 24                                      # the diagonal does: 5000**2
    assert gr.GenericRows(2, (rows, cols, np.array([1, 0.5, 1], np.float32), rhs)).exact_in_fp32() == np.inf
    assert ok.exact_in_fp32(np.array([1.0, 0.25])) == np.inf
    assert ok.exact_in_fp32(np.array([2.0 ** 24, 0.0])) >= 2 ** 24
    # a cancelling run is judged by its partial sums, not by its sum
    run = gr.GenericRows(1, (np.zeros(4, int), np.zeros(4, int), np.array([2 ** 23, 2 ** 23, -2 ** 23, -2 ** 23], np.float32),
                             np.ones(1, np.float32)))
    assert run.exact_in_fp32() >= 2 ** 24
