"""Numpy restatement of the dual-contouring contract (include/fi_hip.h fi_dual_contour): test
infrastructure only.  Every product, sum and quotient is a float32 operation on its own (one rounding each), in the
contract's order, as the device kernels compute them with -ffp-contract=off.  Only numpy.

Lattice arrays are flat, x fastest.  contour() returns (vertices, normals, indices, keys) like field_interpolation_amd.IsoMesh,
plus the number of solves each vertex took and whether it fell back to the cell centre.
"""
import numpy as np

F = np.float32
MAX_SOLVES = 32
REGULARIZATION = F(0.001)


class Unsupported(Exception):
    pass


class NonFinite(Exception):
    pass


def distances(field, iso=0.0):
    """d = f - iso in fp32"""
    return (np.asarray(field, F).reshape(-1) - F(iso)).astype(F)


def calculate_gradients(d, sizes):
    """(N, D) float32: per axis (d[+1] - d[-1]) / 2, one-sided at that axis's own border (the reference's
    calculate_gradients, with the y border at height - 1)"""
    D = len(sizes)
    a = np.asarray(d, F).reshape(tuple(int(s) for s in sizes[::-1]))
    g = np.zeros((D,) + a.shape, F)
    for k in range(D):
        ax = D - 1 - k
        n = a.shape[ax]
        if n < 2:
            continue
        sl = lambda lo, hi: tuple(slice(lo, hi) if i == ax else slice(None) for i in range(D))  # noqa: E731
        out = g[k]
        out[sl(1, n - 1)] = (a[sl(2, n)] - a[sl(0, n - 2)]) / F(2)
        out[sl(0, 1)] = a[sl(1, 2)] - a[sl(0, 1)]
        out[sl(n - 1, n)] = a[sl(n - 1, n)] - a[sl(n - 2, n - 1)]
    return np.stack([g[k].reshape(-1) for k in range(D)], axis=1)


def _strides(sizes):
    s = [1]
    for n in sizes[:-1]:
        s.append(s[-1] * int(n))
    return s


def _det3(a):
    """first-row cofactor expansion of a row-major 3 x 3 (9 arrays): (a0 c0 - a1 c1) + a2 c2"""
    c0 = a[4] * a[8] - a[5] * a[7]
    c1 = a[3] * a[8] - a[5] * a[6]
    c2 = a[3] * a[7] - a[4] * a[6]
    return (a[0] * c0 - a[1] * c1) + a[2] * c2


def solve(M, b):
    """Cramer's rule on the accumulated normal equations.  2-D: the reference's solve_lin_eq_2d; 3-D: _det3 of M with column
    k replaced by b, over _det3(M)."""
    D = len(b)
    if D == 2:
        det = M[0] * M[3] - M[1] * M[2]
        return [(b[0] * M[3] - M[1] * b[1]) / det, (b[1] * M[0] - M[2] * b[0]) / det]
    det = _det3(M)
    out = []
    for k in range(3):
        A = [b[r] if c == k else M[3 * r + c] for r in range(3) for c in range(3)]
        out.append(_det3(A) / det)
    return out


def contour(field, sizes, iso=0.0, gradients=None):
    """-> (vertices (V, D) f32, normals (V, D) f32, indices (P, D) int32, keys (V,) int64, solves (V,) int, fallback (V,) bool)"""
    sizes = [int(s) for s in sizes]
    D = len(sizes)
    if D == 1:
        raise Unsupported("1-D lattice")
    if D not in (2, 3):
        raise ValueError("ndim must be 2 or 3")
    d = distances(field, iso)
    if d.size != int(np.prod(sizes)):
        raise ValueError("field size")
    empty = (np.zeros((0, D), F), np.zeros((0, D), F), np.zeros((0, D), np.int32), np.zeros(0, np.int64),
             np.zeros(0, np.int64), np.zeros(0, bool))
    if min(sizes) < 2:  # no cell: nothing is read
        return empty
    if not np.isfinite(d).all():
        raise NonFinite("non-finite value")
    g = calculate_gradients(d, sizes) if gradients is None else np.asarray(gradients, F).reshape(-1, D)
    st = _strides(sizes)
    inside = d <= F(0)

    # every cell (lowest corner c, c_k <= n_k - 2), ascending linear index of c
    cg = np.meshgrid(*[np.arange(n - 1) for n in sizes[::-1]], indexing="ij")
    cell = np.stack([cg[D - 1 - k].reshape(-1) for k in range(D)], axis=1).astype(np.int64)
    cidx = sum(cell[:, k] * st[k] for k in range(D))
    corner = [cidx + sum(((i >> k) & 1) * st[k] for k in range(D)) for i in range(1 << D)]
    cin = np.stack([inside[c] for c in corner], axis=1)
    active = cin.any(axis=1) & ~cin.all(axis=1)
    cell, cidx, cin = cell[active], cidx[active], cin[active]
    corner = [c[active] for c in corner]
    nv = len(cidx)
    if nv == 0:
        return empty

    # rows: corners (zero where no cell edge at the corner crosses), then D regularisation rows
    zero = np.zeros(nv, F)
    A, b = [], []
    for i in range(1 << D):
        cross = np.zeros(nv, bool)
        for k in range(D):
            cross |= cin[:, i] != cin[:, i ^ (1 << k)]
        gi = [np.where(cross, g[corner[i], k], zero) for k in range(D)]
        s = F((i >> 0) & 1) * gi[0] + F((i >> 1) & 1) * gi[1]
        if D == 3:
            s = s + F((i >> 2) & 1) * gi[2]
        b.append(np.where(cross, s - d[corner[i]], zero))
        A.append(gi)
    # A^T A and A^T b over the corner rows, in row order
    M = [np.zeros(nv, F) for _ in range(D * D)]
    r = [np.zeros(nv, F) for _ in range(D)]
    for i in range(1 << D):
        for j in range(D):
            for k in range(D):
                M[D * j + k] = M[D * j + k] + A[i][j] * A[i][k]
            r[j] = r[j] + A[i][j] * b[i]

    v = [np.full(nv, np.nan, F) for _ in range(D)]
    solves = np.zeros(nv, np.int64)
    going = np.ones(nv, bool)
    reg = np.full(nv, REGULARIZATION, F)
    for _ in range(MAX_SOLVES):
        Mi, ri = list(M), list(r)
        for row in range(D):  # r e_row, right-hand side 0.5 r
            Arow = [np.where(np.full(nv, k == row), reg, zero) for k in range(D)]
            brow = F(0.5) * reg
            for j in range(D):
                for k in range(D):
                    Mi[D * j + k] = Mi[D * j + k] + Arow[j] * Arow[k]
                ri[j] = ri[j] + Arow[j] * brow
        with np.errstate(all="ignore"):
            x = solve(Mi, ri)
        for k in range(D):
            v[k] = np.where(going, x[k], v[k])
        solves += going
        reg = reg * F(2)
        with np.errstate(invalid="ignore"):
            out = np.zeros(nv, bool)
            for k in range(D):
                out |= (v[k] < F(0)) | (v[k] > F(1))
        going &= out
        if not going.any():
            break
    vv = np.stack(v, axis=1)
    with np.errstate(invalid="ignore"):
        accepted = np.isfinite(vv).all(axis=1) & (vv >= F(0)).all(axis=1) & (vv <= F(1)).all(axis=1)
    vv = np.where(accepted[:, None], vv, F(0.5)).astype(F)
    verts = (cell.astype(F) + vv).astype(F)

    # normals: corner gradients interpolated with fi_sample's linear weights at the in-cell offset, then normalised
    u = [(F(1) - vv[:, k], vv[:, k]) for k in range(D)]
    nrm = []
    for c in range(D):
        acc = None
        for i in range(1 << D):
            w = u[0][i & 1]
            for k in range(1, D):
                w = w * u[k][(i >> k) & 1]
            term = w * g[corner[i], c]
            acc = term if acc is None else acc + term
        nrm.append(acc)
    len2 = np.zeros(nv, F)
    for c in range(D):
        len2 = len2 + nrm[c] * nrm[c]
    ln = np.sqrt(len2)
    with np.errstate(all="ignore"):
        nrm = np.stack([np.where(ln > F(0), n / ln, F(0)) for n in nrm], axis=1).astype(F)

    # primitives, cell by cell in ascending index, axis a from D - 1 down to 0
    vid = np.full(int(np.prod(sizes)), -1, np.int64)
    vid[cidx] = np.arange(nv)
    prims = []  # (cell rank, order within the cell, vertices...)
    ext = np.array(sizes, np.int64)
    for a in range(D - 1, -1, -1):
        others = [k for k in range(D) if k != a]
        ok = np.ones(nv, bool)
        for k in others:
            ok &= cell[:, k] <= ext[k] - 3
        p = cidx + sum(st[k] for k in others)
        near, far = inside[p], inside[p + st[a]]
        ok &= near != far
        rows = np.nonzero(ok)[0]
        base = cidx[rows]
        if D == 2:
            nb = vid[base + st[others[0]]]
            me = rows
            if a == 1:  # the +x neighbour: (this, neighbour) when the far end is inside
                seg = np.where(far[rows, None], np.stack([me, nb], 1), np.stack([nb, me], 1))
            else:       # the +y neighbour: (neighbour, this) when the far end is inside
                seg = np.where(far[rows, None], np.stack([nb, me], 1), np.stack([me, nb], 1))
            prims.append((rows, np.full(len(rows), D - 1 - a), seg))
        else:
            bb, cc = (a + 1) % 3, (a + 2) % 3
            q0 = vid[base]
            q1 = vid[base + st[bb]]
            q2 = vid[base + st[bb] + st[cc]]
            q3 = vid[base + st[cc]]
            keep = near[rows, None]
            t0 = np.where(keep, np.stack([q0, q1, q2], 1), np.stack([q0, q3, q2], 1))
            t1 = np.where(keep, np.stack([q0, q2, q3], 1), np.stack([q0, q2, q1], 1))
            o = 2 * (D - 1 - a)
            prims.append((rows, np.full(len(rows), o), t0))
            prims.append((rows, np.full(len(rows), o + 1), t1))
    rk = np.concatenate([p[0] for p in prims])
    od = np.concatenate([p[1] for p in prims])
    ix = np.concatenate([p[2] for p in prims]).reshape(-1, D)
    order = np.lexsort((od, rk))
    idx = ix[order].astype(np.int32)
    return verts, nrm, idx, cidx.astype(np.int64), solves, ~accepted
