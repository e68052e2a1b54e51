"""Numpy restatement of the generic-row path (fi_add_rows_coo -> fi_generic.hip): triplets (row, col, value) in one or more
batches whose row numbers restart per batch, one rhs per row.  Duplicate (row, col) entries are folded left to right in
input order, in float32 or float64, as Eigen's setFromTriplets does after a stable sort; everything derived from the folded
entries (A^T b, diag(A^T A), A^T A x) is evaluated in float64.  Only numpy: no oracle library, no scipy."""
import numpy as np


def fold_runs(values, start, length, dtype):
    """sum of values[start[i] : start[i] + length[i]] for every run i, added strictly left to right in `dtype`
    (np.add.accumulate along rows of equal-length runs is sequential; np.sum and np.add.reduceat add pairwise)"""
    v = np.asarray(values).astype(dtype)
    out = np.empty(len(start), dtype)
    for L in np.unique(length):
        sel = np.flatnonzero(length == L)
        if L == 1:
            out[sel] = v[start[sel]]
            continue
        block = v[start[sel][:, None] + np.arange(L)[None, :]]
        out[sel] = np.cumsum(block, axis=1, dtype=dtype)[:, -1]
    return out


class GenericRows:
    def __init__(self, n_unknowns, batches):
        """batches: one (rows, cols, vals, rhs) or a list of them; rows are numbered from 0 within each batch"""
        if len(batches) == 4 and not isinstance(batches[0], (tuple, list)):
            batches = [batches]
        self.n = int(n_unknowns)
        rows, cols, vals, rhs, off = [], [], [], [], 0
        for r, c, v, b in batches:
            r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
            v, b = np.asarray(v), np.asarray(b)
            assert v.dtype == np.float32 and b.dtype == np.float32, "values and rhs are float32, as fi_triplet's"
            assert len(r) == len(c) == len(v)
            assert len(r) == 0 or (0 <= r.min() and r.max() < len(b) and 0 <= c.min() and c.max() < self.n)
            rows.append(r + off); cols.append(c); vals.append(v); rhs.append(b)
            off += len(b)
        self.rows, self.cols = np.concatenate(rows), np.concatenate(cols)
        self.vals, self.rhs = np.concatenate(vals), np.concatenate(rhs)
        self.m = off
        self._folded = {}

    # ---- duplicates ------------------------------------------------------------------------
    def runs(self):
        """(order, start, length): the stable order by (row, col) and the runs of equal (row, col) in it"""
        key = self.rows * self.n + self.cols
        order = np.argsort(key, kind="stable")
        ks = key[order]
        start = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]]) if len(ks) else np.empty(0, np.int64)
        length = np.diff(np.r_[start, len(ks)])
        return order, start, length

    def fold(self, dtype=np.float64):
        """(rows, cols, values[dtype]) of the unique entries, sorted by (row, col)"""
        dtype = np.dtype(dtype).type
        if dtype not in self._folded:
            order, start, length = self.runs()
            v = fold_runs(self.vals[order], start, length, dtype)
            self._folded[dtype] = (self.rows[order][start], self.cols[order][start], v)
        return self._folded[dtype]

    # ---- normal equations, float64 from the folded entries ------------------------------------
    def _entries(self, dtype):
        r, c, v = self.fold(dtype)
        return r, c, v.astype(np.float64)

    def Atb(self, dtype=np.float64):
        r, c, a = self._entries(dtype)
        return np.bincount(c, weights=a * self.rhs.astype(np.float64)[r], minlength=self.n)

    def diag(self, dtype=np.float64):
        r, c, a = self._entries(dtype)
        return np.bincount(c, weights=a * a, minlength=self.n)

    def apply(self, x, dtype=np.float64):
        """A^T (A x)"""
        r, c, a = self._entries(dtype)
        t = np.bincount(r, weights=a * np.asarray(x, np.float64)[c], minlength=self.m)
        return np.bincount(c, weights=a * t[r], minlength=self.n)

    # ---- error scales: sums of absolute values over the RAW triplets (a run that cancels still rounds at its terms' size) ----
    def _abs_entries(self):
        order, start, _ = self.runs()
        mag = np.add.reduceat(np.abs(self.vals[order].astype(np.float64)), start) if len(start) else np.empty(0)
        return self.rows[order][start], self.cols[order][start], mag

    def abs_apply(self, ax):
        """|A|^T |A| |x| with |A|_rc = sum of |a| over the duplicates of (r, c): the size of what A^T A x adds up"""
        r, c, a = self._abs_entries()
        t = np.bincount(r, weights=a * np.abs(np.asarray(ax, np.float64))[c], minlength=self.m)
        return np.bincount(c, weights=a * t[r], minlength=self.n)

    def abs_Atb(self):
        r, c, a = self._abs_entries()
        return np.bincount(c, weights=a * np.abs(self.rhs.astype(np.float64))[r], minlength=self.n)

    def abs_diag(self):
        r, c, a = self._abs_entries()
        return np.bincount(c, weights=a * a, minlength=self.n)

    # ---- generate_error_map: per triplet, duplicates NOT summed ---------------------------------
    def error_map(self, x):
        """every triplet blames its column with a^2 / sum_row a^2 * res_row^2, res = rhs - sum_row a x"""
        a = self.vals.astype(np.float64)
        x = np.asarray(x, np.float64)
        res = self.rhs.astype(np.float64) - np.bincount(self.rows, weights=a * x[self.cols], minlength=self.m)
        sq = np.bincount(self.rows, weights=a * a, minlength=self.m)
        ok = sq[self.rows] > 0
        w = np.zeros(len(a))
        w[ok] = a[ok] * a[ok] / sq[self.rows[ok]] * res[self.rows[ok]] ** 2
        return np.bincount(self.cols, weights=w, minlength=self.n)

    def abs_error_map(self, x):
        """Error scale of error_map per column: the blame terms are non-negative, so their sum is its own scale; a rounding
        of relative size e in the row residual (which adds up mag = |rhs| + sum |a x|) moves res^2 by 2 |res| e mag."""
        a = self.vals.astype(np.float64)
        x = np.asarray(x, np.float64)
        ax = np.bincount(self.rows, weights=a * x[self.cols], minlength=self.m)
        mag = np.abs(self.rhs.astype(np.float64)) + np.bincount(self.rows, weights=np.abs(a * x[self.cols]), minlength=self.m)
        res = self.rhs.astype(np.float64) - ax
        sq = np.bincount(self.rows, weights=a * a, minlength=self.m)
        ok = sq[self.rows] > 0
        w = np.zeros(len(a))
        w[ok] = a[ok] * a[ok] / sq[self.rows[ok]] * (2.0 * np.abs(res[self.rows[ok]]) * mag[self.rows[ok]] + res[self.rows[ok]] ** 2)
        return np.bincount(self.cols, weights=w, minlength=self.n)

    # ---- the tile operator of k_generic_tile ---------------------------------------------------
    def tile_apply(self, x, sizes, ts, dtype=np.float64):
        """y_i = sum_r a_ri sum_{j in row r, tile(j) == tile(i)} a_rj x_j: entry (i, j) of A^T A survives only when i and j
        share a ts^D tile of the lattice `sizes` (x fastest)"""
        r, c, a = self._entries(dtype)
        tile = tile_index(sizes, ts)[c]
        ntile = int(tile.max()) + 1 if len(tile) else 1
        piece = r * ntile + tile                                     # one partial row per (row, tile)
        uniq, inv = np.unique(piece, return_inverse=True)
        u = np.bincount(inv, weights=a * np.asarray(x, np.float64)[c], minlength=len(uniq))
        return np.bincount(c, weights=a * u[inv], minlength=self.n)

    # ---- exactness guard -------------------------------------------------------------------
    def exact_in_fp32(self, x=None):
        """The largest absolute value any intermediate of fold, A x, A^T t, A^T b and diag(A^T A) can take whatever the
        order of the additions, in int64 / float64: within a run of duplicates the larger of the sums of its positive and of
        its negative values (no partial sum of any subset exceeds it); for the products the sums of absolute values of the
        terms, built on the folded entries.  inf if a value, a rhs or x is not an integer.  Below 2**24 every partial sum
        is an integer float32 holds exactly, so every order of additions gives the same bits."""
        x = np.ones(self.n) if x is None else np.asarray(x, np.float64)
        a, b = self.vals.astype(np.float64), self.rhs.astype(np.float64)
        if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(np.isfinite(x))
                and np.all(a == np.rint(a)) and np.all(b == np.rint(b)) and np.all(x == np.rint(x))):
            return float("inf")
        if max(np.abs(a).max(initial=0), np.abs(b).max(initial=0), np.abs(x).max(initial=0)) >= 2.0 ** 62 / max(1, len(a)):
            return float("inf")                                       # (the int64 sums below would overflow)
        worst = max(float(np.abs(b).max(initial=0)), float(np.abs(x).max(initial=0)))
        if len(a):
            order, start, length = self.runs()
            ai = a[order].astype(np.int64)
            pos = np.add.reduceat(np.maximum(ai, 0), start)           # integers: exact in any order
            neg = np.add.reduceat(np.maximum(-ai, 0), start)
            folded = np.abs(pos - neg).astype(np.float64)
            r, c = self.rows[order][start], self.cols[order][start]
            t_abs = np.bincount(r, weights=folded * np.abs(x)[c], minlength=self.m)
            y_abs = np.bincount(c, weights=folded * t_abs[r], minlength=self.n)
            b_abs = np.bincount(c, weights=folded * np.abs(b)[r], minlength=self.n)
            d_abs = np.bincount(c, weights=folded * folded, minlength=self.n)
            worst = max(worst, float(np.maximum(pos, neg).max()), float(t_abs.max()), float(y_abs.max()),
                        float(b_abs.max()), float(d_abs.max()))
        return worst

    # ---- chain lengths for derived tolerances ------------------------------------------------
    def chain_lengths(self):
        """(longest duplicate run, longest row, longest column) in entries; rows and columns counted over the raw triplets
        (an upper bound of the folded counts, and what the error map walks)"""
        _, _, length = self.runs()
        row = np.bincount(self.rows, minlength=self.m).max() if len(self.rows) else 0
        col = np.bincount(self.cols, minlength=self.n).max() if len(self.cols) else 0
        return int(length.max()) if len(length) else 0, int(row), int(col)


def tile_index(sizes, ts):
    """tile number of every unknown of the lattice `sizes` (x fastest), tiles of ts along every axis"""
    n = int(np.prod(sizes))
    j = np.arange(n, dtype=np.int64)
    t, mul = np.zeros(n, np.int64), 1
    for s in sizes:
        t += ((j % s) // ts) * mul
        mul *= (s + ts - 1) // ts
        j //= s
    return t


def order_sensitive_runs(rng, nruns, dtype=np.float32, lo=3, hi=40):
    """Runs of `lo` to `hi` duplicate values whose sum depends on the order of the additions in `dtype`: terms of the size
    of 2**p (p = 24 for float32, 53 for float64: the first power of two above which odd integers are not representable),
    once or twice that, and units 1 and 3, with signs.  Every value is a float32 (the triplet format) and an integer, and
    every partial sum stays far below overflow.  -> (lengths, values[float32] run after run)"""
    p = 24 if np.dtype(dtype) == np.float32 else 53
    lengths = rng.integers(lo, hi + 1, nruns)
    total = int(lengths.sum())
    big = np.float32(2.0 ** p) * rng.choice(np.array([1, 2], np.float32), total)
    unit = rng.choice(np.array([1, 3], np.float32), total)
    v = np.where(rng.random(total) < 0.3, big, unit) * rng.choice(np.array([-1, 1], np.float32), total)
    # every run opens with  1, 1, 2**p : (1 + 1) + 2**p keeps the 2, 1 + (1 + 2**p) loses it
    first = np.r_[0, np.cumsum(lengths)[:-1]]
    v[first], v[first + 1], v[first + 2] = 1.0, 1.0, 2.0 ** p
    return lengths, v.astype(np.float32)


# ---- the shipped cases (tests/test_generic_reference.py checks them on the CPU, tests/test_gpu_generic_scale.py runs them) ----

def split_batches(rows, cols, vals, rhs, bounds):
    """The global rows [bounds[k], bounds[k+1]) as batch k, row numbers restarting, triplets in their input order"""
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        sel = (rows >= lo) & (rows < hi)
        out.append((rows[sel] - lo, cols[sel], vals[sel], rhs[lo:hi]))
    return out


def exact_case(seed, n, m, ntrip, structures):
    """Values in {+-1} (and explicit zeros), rhs and x in {-1, 0, 1}, triplets in a random permutation, three batches of
    unequal size.  With `structures`: one row and one column of 50 000 entries, 20 000 empty rows with non-zero rhs (the
    first and last row of every batch among them), 5 000 unknowns no row touches (the first and last among them), 10 000
    explicit zeros, 1 000 rows whose values are all zero, a (row, col) pair repeated 10 000 times whose sum is 0 and one whose
    sum is 400, their copies spread over the batch.  -> (batches, x, names of the structures' rows / columns)"""
    rng = np.random.default_rng(seed)
    bounds = [0, m // 7, m // 7 + m // 3, m]
    rows = rng.integers(0, m, ntrip).astype(np.int64)
    cols = rng.integers(0, n, ntrip).astype(np.int64)
    vals = rng.choice(np.array([-1, 1], np.float32), ntrip)
    rhs = rng.integers(-1, 2, m).astype(np.float32)
    x = rng.integers(-1, 2, n).astype(np.float64)
    info = {}
    if structures:
        special = rng.choice(np.arange(1, m - 1), 20000 + 1000 + 3, replace=False)
        edge = np.array([0, bounds[1] - 1, bounds[1], bounds[2] - 1, bounds[2], m - 1])
        special = special[~np.isin(special, edge)]
        long_row, row_zero_sum, row_sum = special[:3]
        zero_rows = special[3:1003]
        empty = np.r_[edge, special[1003:1003 + 20000 - len(edge)]]
        dead = np.r_[0, n - 1, rng.choice(np.arange(1, n - 1), 4998, replace=False)]
        live = np.setdiff1d(np.arange(n), dead)
        long_col, col_zero_sum, col_sum = rng.choice(live, 3, replace=False)
        keep = ~np.isin(rows, np.r_[empty, long_row, row_zero_sum, row_sum]) & ~np.isin(cols, dead)
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
        vals[rng.choice(len(vals), 10000, replace=False)] = 0.0
        vals[np.isin(rows, zero_rows)] = 0.0
        rhs[empty] = rng.choice(np.array([-1, 1], np.float32), len(empty))
        rhs[zero_rows] = 1.0
        free_rows = np.setdiff1d(np.arange(m), np.r_[empty, special[:3], zero_rows])
        add_r = [np.full(50000, long_row), rng.choice(free_rows, 50000, replace=False),
                 np.full(10000, row_zero_sum), np.full(10000, row_sum), zero_rows]
        add_c = [rng.choice(live, 50000, replace=False), np.full(50000, long_col),
                 np.full(10000, col_zero_sum), np.full(10000, col_sum), rng.choice(live, len(zero_rows))]
        add_v = [rng.choice(np.array([-1, 1], np.float32), 50000), rng.choice(np.array([-1, 1], np.float32), 50000),
                 rng.permutation(np.r_[np.ones(5000, np.float32), -np.ones(5000, np.float32)]),
                 rng.permutation(np.r_[np.ones(5200, np.float32), -np.ones(4800, np.float32)]),
                 np.zeros(len(zero_rows), np.float32)]          # (so that none of the all-zero rows is an empty one)
        rows = np.r_[rows, np.concatenate(add_r)]
        cols = np.r_[cols, np.concatenate(add_c)]
        vals = np.r_[vals, np.concatenate(add_v)].astype(np.float32)
        perm = rng.permutation(len(rows))
        rows, cols, vals = rows[perm], cols[perm], vals[perm]
        info = dict(long_row=int(long_row), long_col=int(long_col), empty_rows=empty, dead_cols=dead, zero_rows=zero_rows,
                    zero_sum=(int(row_zero_sum), int(col_zero_sum)), sum_400=(int(row_sum), int(col_sum)))
    return split_batches(rows, cols, vals, rhs, bounds), x, info


def order_case(seed, nruns, dtype):
    """`nruns` order-sensitive runs (order_sensitive_runs), run r on (row r, column r) with rhs[r] = 1, so that (A^T b)[r] is
    the folded value itself.  The triplets are shuffled across runs; each run keeps its relative order.  One batch."""
    rng = np.random.default_rng(seed)
    lengths, v = order_sensitive_runs(rng, nruns, dtype)
    ids = np.repeat(np.arange(nruns, dtype=np.int64), lengths)
    shuffled = rng.permutation(ids)
    where = np.argsort(shuffled, kind="stable")       # the positions run 0 gets, ascending, then run 1's, ...
    vals = np.empty(len(v), np.float32)
    vals[where] = v
    return (shuffled, shuffled.copy(), vals, np.ones(nruns, np.float32)), lengths


def real_case(seed, n, m, ntrip, dup=0.05):
    """Normal values, a fraction `dup` of the triplets repeating the (row, col) of another one, rows and columns short
    (uniform draws), three batches of unequal size.  -> (batches, x[float32-valued])"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, m, ntrip).astype(np.int64)
    cols = rng.integers(0, n, ntrip).astype(np.int64)
    again = rng.choice(ntrip, int(dup * ntrip), replace=False)
    src = rng.integers(0, ntrip, len(again))
    rows[again], cols[again] = rows[src], cols[src]
    vals = rng.normal(size=ntrip).astype(np.float32)
    rhs = rng.normal(size=m).astype(np.float32)
    x = rng.normal(size=n).astype(np.float32).astype(np.float64)
    return split_batches(rows, cols, vals, rhs, [0, m // 7, m // 7 + m // 3, m]), x


def smooth_case(seed, n, w=0.25):
    """One unit-weight data row per unknown plus second-difference rows of weight `w`: A^T A = I + w^2 D^T D, whose
    eigenvalues lie in [1, 1 + 16 w^2] -- conditioning bounded by construction.  Two batches."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    data = (i, i, np.ones(n, np.float32), rng.normal(size=n).astype(np.float32))
    k = np.arange(1, n - 1, dtype=np.int64)
    r2 = np.repeat(k - 1, 3)
    c2 = np.stack([k - 1, k, k + 1], 1).ravel()
    v2 = np.tile(np.array([w, -2 * w, w], np.float32), len(k))
    return [data, (r2, c2, v2, np.zeros(len(k), np.float32))]
