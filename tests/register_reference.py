"""Numpy restatement of the contract of fi_mesh_register / fi_points_register (include/fi_hip.h): rigid
registration of a point cloud to a mesh or to a point set by iterated closest points.  Test infrastructure, independent of the
device code.  Every floating-point step is written the way the contract states it -- fp64 from the fp32 inputs, one rounding
per operation, no sin / cos / atan -- so that the transform, the figures and the arrays returned are the bytes the device must
produce.  The pairs come through tests/surface_reference.py (fi_surface_distance's restatement) and
tests/nearest_reference.py (fi_points_nearest's); the block sums are tests/meshpts_reference.py's tree_sum.  Only numpy."""
import numpy as np

import nearest_reference as NR
import surface_reference as SR
from meshpts_reference import face_normals, tree_sum

PLANE, POINT = 0, 1
MODES = {"plane": PLANE, "point": POINT}
NONE, HUBER, CAUCHY, TUKEY = -1, 0, 1, 2
LOSSES = {None: NONE, "huber": HUBER, "cauchy": CAUCHY, "tukey": TUKEY}
TUNING = {HUBER: np.float32(1.345), CAUCHY: np.float32(2.385), TUKEY: np.float32(4.685)}
F64 = np.float64


class Invalid(Exception):
    """what the device answers with FI_ERR_INVALID"""


def unknowns(D):
    return 6 if D == 3 else 3


def start(D, initial):
    """(R (D, D), t (D,)) float64 from `initial` ((D + 1, D + 1), last row ignored) or the identity"""
    if initial is None:
        return np.eye(D, dtype=F64), np.zeros(D, F64)
    T = np.asarray(initial, F64).reshape(D + 1, D + 1)
    if not np.all(np.isfinite(T[:D])):
        raise Invalid("initial")
    return T[:D, :D].copy(), T[:D, D].copy()


def pivot(source):
    """g0 = 0.5 (lo + hi) + 0.0 of the finite points' box (a zero is +0); zeros without a finite point"""
    x = np.asarray(source, np.float32)
    ok = np.all(np.isfinite(x), axis=1)
    if not ok.any():
        return np.zeros(x.shape[1], F64), False
    lo, hi = x[ok].min(axis=0).astype(F64), x[ok].max(axis=0).astype(F64)
    return 0.5 * (lo + hi) + 0.0, True


def affine(R, t, x):
    """((R[a][0] x0 + R[a][1] x1) + R[a][2] x2) + t[a] per row of x (float64 (n, D)) -> float64 (n, D)"""
    D = len(t)
    out = np.empty(x.shape, F64)
    with np.errstate(all="ignore"):
        for a in range(D):
            s = R[a, 0] * x[:, 0] + R[a, 1] * x[:, 1]
            if D == 3:
                s = s + R[a, 2] * x[:, 2]
            out[:, a] = s + t[a]
    return out


def transformed(R, t, source):
    with np.errstate(all="ignore"):
        return affine(R, t, np.asarray(source, np.float32).astype(F64)).astype(np.float32)


class Target:
    """a mesh (vertices, indices) or a point set (points, normals or None)"""

    def __init__(self, vertices=None, indices=None, points=None, normals=None):
        self.mesh = vertices is not None
        if self.mesh:
            self.v = np.asarray(vertices, np.float32)
            self.D = self.v.shape[1]
            self.i = np.asarray(indices, np.int64).reshape(-1, self.D)
        else:
            self.v = np.asarray(points, np.float32)
            self.D = self.v.shape[1]
            self.n = None if normals is None else np.asarray(normals, np.float32)

    def pair(self, p, max_distance):
        """(d float32 (n,), j int64 (n,), c float32 (n, D))"""
        if self.mesh:
            return SR.distance(self.v, self.i, p, self.D, max_distance)
        d, j = NR.nearest(self.v, p, self.D, max_distance)
        c = np.full(p.shape, np.nan, np.float32)
        c[j >= 0] = self.v[j[j >= 0]]
        return d, j, c

    def normals(self, j):
        """(unit normals float64 (m, D), good (m,)) of the primitives / target points j (all >= 0)"""
        with np.errstate(all="ignore"):
            if self.mesh:
                n, w = face_normals(self.v, self.i[j])
            else:
                n = self.n[j].astype(F64)
                w = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]
                if self.D == 3:
                    w = w + n[:, 2] * n[:, 2]
                w = np.sqrt(w)
            good = np.isfinite(w) & (w != 0.0)
            return n / w[:, None], good


def weights(rho, loss, tuning, scale):
    """w of every pair from rho (float64): 1 without a loss, else 4.10's formulas in double with u = rho / (s c)"""
    if loss == NONE:
        return np.ones(len(rho), F64)
    c = np.float32(tuning) if tuning > 0 else TUNING[loss]
    sc = F64(np.float32(scale)) * F64(c)
    with np.errstate(all="ignore"):
        u = rho / sc
        if loss == HUBER:
            return np.where(u <= 1.0, 1.0, 1.0 / u)
        if loss == CAUCHY:
            return 1.0 / (1.0 + u * u)
        t = 1.0 - u * u
        return np.where(u < 1.0, t * t, 0.0)


def rows(D, mode, u, e, n):
    """the Jacobian rows J (rows, m, U), the residuals r (rows, m) and rho (m,) of counted pairs"""
    m = len(u)
    z, one = np.zeros(m, F64), np.ones(m, F64)
    with np.errstate(all="ignore"):
        if mode == PLANE:
            if D == 3:
                r = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
                J = [u[:, 1] * n[:, 2] - u[:, 2] * n[:, 1], u[:, 2] * n[:, 0] - u[:, 0] * n[:, 2],
                     u[:, 0] * n[:, 1] - u[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]]
            else:
                r = n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]
                J = [u[:, 0] * n[:, 1] - u[:, 1] * n[:, 0], n[:, 0], n[:, 1]]
            return np.stack(J, axis=1)[None], r[None], np.abs(r)
        if D == 3:
            J = [[z, u[:, 2], -u[:, 1], one, z, z], [-u[:, 2], z, u[:, 0], z, one, z], [u[:, 1], -u[:, 0], z, z, z, one]]
            rho = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        else:
            J = [[-u[:, 1], one, z], [u[:, 0], z, one]]
            rho = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
        return np.stack([np.stack(j, axis=1) for j in J]), e.T.copy(), rho


def _over_rows(terms):
    s = terms[0]
    for a in range(1, len(terms)):
        s = s + terms[a]
    return s


def evaluate(target, source, R, t, g0, mode, max_distance, loss, tuning, scale):
    """items 2 to 6: the transformed points, the pairs, the sums and the counts"""
    D = target.D
    U = unknowns(D)
    x = np.asarray(source, np.float32)
    n = len(x)
    p = transformed(R, t, x)
    g = affine(R, t, g0[None])[0]
    d, j, c = target.pair(p, np.float32(max_distance))
    finite = np.isfinite(d)
    out = {"p": p, "d": d, "g": g, "queries": n, "invalid": int(np.isnan(d).sum())}
    out["beyond"] = n - int(finite.sum()) - out["invalid"]
    counted = finite.copy()
    nrm = np.zeros((n, D), F64)
    if mode == PLANE:
        k = np.flatnonzero(finite)
        unit, good = target.normals(j[k])
        nrm[k] = unit
        counted[k[~good]] = False
    out["counted"] = int(counted.sum())
    out["degenerate"] = int(finite.sum()) - out["counted"]
    k = np.flatnonzero(counted)
    M, b = np.zeros((U, U), F64), np.zeros(U, F64)
    with np.errstate(all="ignore"):
        p64 = p[k].astype(F64)
        u, e = p64 - g[None], p64 - c[k].astype(F64)
        J, r, rho = rows(D, mode, u, e, nrm[k])
        w = weights(rho, loss, tuning, scale)

        def total(per_pair):
            full = np.zeros(n, F64)
            full[k] = per_pair
            return tree_sum(full) if n else F64(0.0)

        for a in range(U):
            for bb in range(a, U):
                M[a, bb] = total(w * _over_rows([J[q][:, a] * J[q][:, bb] for q in range(len(J))]))
            b[a] = total(w * _over_rows([J[q][:, a] * r[q] for q in range(len(J))]))
        sq = _over_rows([r[q] * r[q] for q in range(len(J))])
        out["M"], out["b"], out["Sw"], out["S"] = M, b, total(w * sq), total(sq)
    return out


def solve(M, b):
    """M delta = -b by the contract's Cholesky (M: its upper triangle) -> (delta, fixed_mask)"""
    U = len(b)
    with np.errstate(all="ignore"):
        top = M[0, 0]
        for j in range(1, U):
            top = M[j, j] if M[j, j] > top else top
        lim = 1e-12 * top
        L = np.zeros((U, U), F64)
        free, mask = [], 0
        for j in range(U):
            d = M[j, j]
            for k in free:
                d = d - L[j, k] * L[j, k]
            if not d > lim:
                mask |= 1 << j
                continue
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, U):
                s = M[j, i]
                for k in free:
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
            free.append(j)
        y, delta = np.zeros(U, F64), np.zeros(U, F64)
        for j in free:
            s = -b[j]
            for k in free:
                if k < j:
                    s = s - L[j, k] * y[k]
            y[j] = s / L[j, j]
        for j in reversed(free):
            s = y[j]
            for k in reversed(free):
                if k > j:
                    s = s - L[k, j] * delta[k]
            delta[j] = s / L[j, j]
    return delta, mask


def cayley(D, omega):
    """the rotation of a step: exact for any omega, I + [omega]x to first order"""
    with np.errstate(all="ignore"):
        if D == 2:
            a = 0.5 * omega[0]
            a2 = a * a
            den = 1.0 + a2
            c, s = (1.0 - a2) / den, (2.0 * a) / den
            return np.array([[c, -s], [s, c]], F64)
        v = [0.5 * omega[0], 0.5 * omega[1], 0.5 * omega[2]]
        q = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        den, c0 = 1.0 + q, 1.0 - q
        N = np.empty((3, 3), F64)
        for a in range(3):
            N[a, a] = c0 + 2.0 * (v[a] * v[a])
        N[0, 1] = 2.0 * (v[0] * v[1]) - 2.0 * v[2]
        N[1, 0] = 2.0 * (v[0] * v[1]) + 2.0 * v[2]
        N[0, 2] = 2.0 * (v[0] * v[2]) + 2.0 * v[1]
        N[2, 0] = 2.0 * (v[0] * v[2]) - 2.0 * v[1]
        N[1, 2] = 2.0 * (v[1] * v[2]) - 2.0 * v[0]
        N[2, 1] = 2.0 * (v[1] * v[2]) + 2.0 * v[0]
        return N / den


def update(D, R, t, g, delta):
    """t <- (R_d (t - g) + g) + tau, R <- R_d R, row-by-column sums in ascending index"""
    nrot = 3 if D == 3 else 1
    Rd = cayley(D, delta[:nrot])
    tau = delta[nrot:]
    with np.errstate(all="ignore"):
        h = t - g
        R2, t2 = np.empty((D, D), F64), np.empty(D, F64)
        for a in range(D):
            s = Rd[a, 0] * h[0] + Rd[a, 1] * h[1]
            if D == 3:
                s = s + Rd[a, 2] * h[2]
            t2[a] = (s + g[a]) + tau[a]
            for c in range(D):
                s = Rd[a, 0] * R[0, c] + Rd[a, 1] * R[1, c]
                if D == 3:
                    s = s + Rd[a, 2] * R[2, c]
                R2[a, c] = s
    return R2, t2


def register(target, source, mode=PLANE, max_iterations=30, max_distance=np.inf, rotation_tolerance=1e-6,
             translation_tolerance=1e-6, loss=NONE, tuning=0.0, scale=0.0, initial=None, history=None):
    """-> the dict of fi_registration's fields plus "transformed" (n, D) float32 and "distances" (n,) float32.  history: a
    list that receives (rms, weighted_rms) of the evaluation before every step"""
    D = target.D
    x = np.asarray(source, np.float32).reshape(-1, D)
    md = np.float32(max_distance)
    bad = lambda v: not v >= 0   # noqa: E731  (NaN fails)
    if mode not in (PLANE, POINT) or loss not in (NONE, HUBER, CAUCHY, TUKEY) or max_iterations < 0 or bad(md) or \
            bad(rotation_tolerance) or bad(translation_tolerance) or (loss != NONE and not np.float32(scale) > 0) or \
            (loss != NONE and bad(np.float32(tuning))) or (mode == PLANE and not target.mesh and target.n is None):
        raise Invalid("arguments")
    R, t = start(D, initial)
    nrot = 3 if D == 3 else 1
    g0, any_finite = pivot(x) if len(x) else (np.zeros(D, F64), False)
    out = {"iterations": 0, "converged": 0, "fixed_mask": 0, "last_rotation": 0.0, "last_translation": 0.0}
    limit = max_iterations if any_finite else 0
    while out["iterations"] < limit:
        ev = evaluate(target, x, R, t, g0, mode, md, loss, tuning, scale)
        if history is not None:
            history.append(_rms(ev, D, mode))
        if ev["counted"] == 0:
            break
        delta, out["fixed_mask"] = solve(ev["M"], ev["b"])
        R, t = update(D, R, t, ev["g"], delta)
        out["iterations"] += 1
        out["last_rotation"] = float(np.max(np.abs(delta[:nrot])))
        out["last_translation"] = float(np.max(np.abs(delta[nrot:])))
        if out["last_rotation"] <= rotation_tolerance and out["last_translation"] <= translation_tolerance:
            out["converged"] = 1
            break
    ev = evaluate(target, x, R, t, g0, mode, md, loss, tuning, scale)
    for k in ("queries", "counted", "beyond", "invalid", "degenerate"):
        out[k] = ev[k]
    out["rms"], out["weighted_rms"] = _rms(ev, D, mode)
    T = np.zeros((D + 1, D + 1), F64)
    T[:D, :D], T[:D, D], T[D, D] = R, t, 1.0
    out["transform"] = T
    out["transformed"], out["distances"] = ev["p"], ev["d"]
    return out


def _rms(ev, D, mode):
    if ev["counted"] == 0:
        return 0.0, 0.0
    rows_ = F64(ev["counted"] if mode == PLANE else D * ev["counted"])
    with np.errstate(all="ignore"):
        return float(np.sqrt(ev["S"] / rows_)), float(np.sqrt(ev["Sw"] / rows_))


# ---- shapes the tests share ---------------------------------------------------------------------------------------------

def rotation(axis, degrees):
    """an fp64 Rodrigues matrix (for test inputs only: the contract itself uses no sin / cos)"""
    k = np.asarray(axis, F64)
    k = k / np.linalg.norm(k)
    a = np.deg2rad(degrees)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], F64)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def moved(points, Rs, shift):
    """the source of a test: `points` turned by Rs about their centroid and shifted, in fp32"""
    p = np.asarray(points, F64)
    c = p.mean(axis=0)
    return ((p - c) @ Rs.T + c + np.asarray(shift, F64)).astype(np.float32)


def truth(points, Rs, shift):
    """(R, t) of the registration that undoes `moved`: p = Rs^T (x - c - shift) + c"""
    c = np.asarray(points, F64).mean(axis=0)
    return Rs.T, c - Rs.T @ (c + np.asarray(shift, F64))


def rotation2(degrees):
    a = np.deg2rad(degrees)
    return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], F64)


def cube_case(n=600, degrees=8.0, seed=7):
    """4.15's cube (866 vertices, 1 728 triangles), n sample_mesh points turned about (1, 2, 3) and shifted by (0.6, -0.4, 0.5)
    -> (vertices, triangles, the points on the cube, their face normals, the source, (R, t) of the truth)"""
    import meshpts_reference as P
    import simplify_reference as S
    v, t = S.cube_mesh()
    pts, nrm, _prim = P.sample(v, None, t, n, seed, P.FACE, True)
    Rs, shift = rotation((1, 2, 3), degrees), (0.6, -0.4, 0.5)
    return v, t, pts, nrm, moved(pts, Rs, shift), truth(pts, Rs, shift)


def rectangle_case(n=200, degrees=6.0, seed=3):
    """a closed 32-segment rectangle [2, 12] x [3, 9] (10 + 6 + 10 + 6 segments, counter-clockwise), n points on it turned and
    shifted by (0.3, -0.2) -> as cube_case"""
    import meshpts_reference as P
    pts = [(2.0 + i, 3.0) for i in range(10)] + [(12.0, 3.0 + i) for i in range(6)] + [(12.0 - i, 9.0) for i in range(10)] + \
          [(2.0, 9.0 - i) for i in range(6)]
    v = np.array(pts, np.float32)
    s = np.stack([np.arange(32), (np.arange(32) + 1) % 32], axis=1).astype(np.int32)
    on, nrm, _prim = P.sample(v, None, s, n, seed, P.FACE, True)
    Rs, shift = rotation2(degrees), (0.3, -0.2)
    return v, s, on, nrm, moved(on, Rs, shift), truth(on, Rs, shift)


def flat_case():
    """a flat 9 x 9 grid at z = 3 and its own vertices' copies inside it, tilted 5 degrees about x and lifted 0.4
    -> (vertices, triangles, source)"""
    x, y = np.meshgrid(np.arange(9.0), np.arange(9.0), indexing="xy")
    v = np.stack([x, y, np.full_like(x, 3.0)], axis=2).reshape(-1, 3).astype(np.float32)
    q = np.arange(8)[:, None] * 9 + np.arange(8)[None, :]
    q = q.reshape(-1)
    t = np.concatenate([np.stack([q, q + 1, q + 10], axis=1), np.stack([q, q + 10, q + 9], axis=1)]).astype(np.int32)
    gx, gy = np.meshgrid(1.25 + 0.5 * np.arange(12), 1.25 + 0.5 * np.arange(12), indexing="xy")
    on = np.stack([gx, gy, np.full_like(gx, 3.0)], axis=2).reshape(-1, 3)
    return v, t, moved(on, rotation((1, 0, 0), 5.0), (0.0, 0.0, 0.4))


def outlier_case():
    """cube_case with 60 of its 600 source points moved 3 to 6 units: to a place over the same face of the cube [2.25, 11.25]^3,
    at least 1 inside the face's edges and h in [0.6, 1.4] off it, outwards.  Every one of them then pairs with its own face
    at the truth, with the residual h: beyond Tukey's cut at scale 0.1 (0.4685) and within max_distance 1.5
    -> (vertices, triangles, source, (R, t) of the truth)"""
    v, t, pts, nrm, src, tr = cube_case()
    rng = np.random.default_rng(5)
    src = src.copy()
    Rs = rotation((1, 2, 3), 8.0)
    for k in rng.choice(600, 60, replace=False):
        n, p = nrm[k].astype(F64), pts[k].astype(F64)
        h = rng.uniform(0.6, 1.4)
        while True:
            q = rng.uniform(3.25, 10.25, size=3)
            q = q - n * (n @ (q - p)) + n * h            # over p's face, h off it
            if 3.0 <= np.linalg.norm(q - p) <= 6.0:
                break
        src[k] = (src[k].astype(F64) + Rs @ (q - p)).astype(np.float32)
    return v, t, src, tr
