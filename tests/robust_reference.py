"""Robust fits, restated in numpy (include/fi_hip.h "robust fits"): every operation in the contract's
order and type, so that the GPU results can be compared bit for bit; and the whole loop in fp64 on the oracle's exact solver.

A batch is a dict: pos (n, D); nrm (n, D) or None; pw (n,) or None; val (n,) or None; vw, vk, gw, gk as fi_add_points takes
them; prior=True marks a border-prior batch (not data: left out).  Points are numbered in batch order, then within a batch."""
import numpy as np

F = np.float32
HUBER, CAUCHY, TUKEY = "huber", "cauchy", "tukey"
DEFAULT_TUNING = {HUBER: F(1.345), CAUCHY: F(2.385), TUKEY: F(4.685)}
VALUE_NEAREST, VALUE_LINEAR = 0, 1
GRAD_NEAREST, GRAD_CELL_EDGES, GRAD_LINEAR = 0, 1, 2


def batch(pos, nrm=None, pw=None, val=None, vw=1.0, vk=VALUE_LINEAR, gw=1.0, gk=GRAD_CELL_EDGES, prior=False):
    f = lambda a, shape: None if a is None else np.ascontiguousarray(a, F).reshape(shape)  # noqa: E731
    pos = np.ascontiguousarray(pos, F)
    if pos.ndim != 2:
        pos = pos.reshape(len(pos), -1)
    return dict(pos=pos, nrm=f(nrm, pos.shape), pw=f(pw, -1), val=f(val, -1), vw=F(vw), vk=int(vk), gw=F(gw), gk=int(gk),
                prior=bool(prior))


def _round_half_away(p):
    """roundf of fp32 values, computed exactly in fp64"""
    p64 = p.astype(np.float64)
    return (np.sign(p64) * np.floor(np.abs(p64) + 0.5)).astype(F)


def _point_rows(sizes, b):
    """The rows of every point of a batch at point weight 1 (fi_rows.h): a list of (emitted (n,), origin (n, D) int64,
    c (n, 2^D) float32, rhs (n,) float32), the value row first, then the gradient rows that the batch has."""
    gn = np.asarray(sizes, np.int64)
    D = len(gn)
    NC = 1 << D
    p = b["pos"]
    n = len(p)
    base = np.ones(n, F) if b["pw"] is None else b["pw"]
    value = np.zeros(n, F) if b["val"] is None else b["val"]
    nrm = b["nrm"]
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(p).all(axis=1)
        fl = np.floor(p)
        axis_ok = (fl >= F(-1.0)) & (fl <= (gn - 1).astype(F))
        in_ext = finite & axis_ok.all(axis=1)
        cell = np.where(axis_ok, np.nan_to_num(fl, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(np.int64)
        t = np.where(axis_ok, p - cell.astype(F), F(0)).astype(F)
        cell_valid = in_ext & ((0 <= cell) & (cell + 1 < gn)).all(axis=1)
        rows = []
        # ---- value row
        cw = F(1.0) * b["vw"]
        on = (base * b["vw"]) != 0
        c = np.zeros((n, NC), F)
        origin = cell.copy()
        if b["vk"] == VALUE_LINEAR:
            total = np.zeros(n, F)
            kept = np.zeros(n, np.int64)
            for q in range(NC):
                lw = np.ones(n, F)
                inside = np.ones(n, bool)
                for d in range(D):
                    up = (q >> d) & 1
                    lw = (lw * (t[:, d] if up else F(1.0) - t[:, d])).astype(F)
                    cc = cell[:, d] + up
                    inside &= (0 <= cc) & (cc < gn[d])
                s = (lw * cw).astype(F)
                c[:, q] = np.where(inside, s, F(0))
                total = np.where(inside, total + s, total).astype(F)
                kept += inside
            emitted = on & in_ext & (kept > 0)
            rhs = (total * value).astype(F)
        else:
            r = _round_half_away(np.where(np.isfinite(p), p, F(0)))
            ok = ((r >= 0) & (r <= (gn - 1).astype(F))).all(axis=1)
            qn = np.where(np.isfinite(r), r, 0).astype(np.int64)
            along = np.zeros(n, F)
            corner = np.zeros(n, np.int64)
            for d in range(D):
                along = (along + ((p[:, d] - qn[:, d].astype(F)).astype(F) * (nrm[:, d] * F(1.0)).astype(F)).astype(F)).astype(F)
                bs = np.where(np.isfinite(fl[:, d]), fl[:, d], 0).astype(np.int64)
                bs = np.maximum(bs, -1)
                bs = np.minimum(bs, qn[:, d])
                bs = np.where(qn[:, d] - bs > 1, qn[:, d] - 1, bs)
                origin[:, d] = bs
                corner |= (qn[:, d] - bs) << d
            emitted = on & finite & ok
            corner = np.where(emitted, corner, 0)
            c[np.arange(n), corner] = F(1.0) * cw
            rhs = ((value - along).astype(F) * cw).astype(F)
        rows.append((emitted, origin, c, rhs))
        # ---- gradient rows
        if nrm is not None and b["gw"] != 0:
            if b["gk"] not in (GRAD_NEAREST, GRAD_CELL_EDGES):
                raise ValueError("robust fits do not cover the linear-interpolation gradient kernel")
            cw = F(1.0) * b["gw"]
            emitted = ((base * b["gw"]) != 0) & cell_valid
            for d in range(D):
                gd = (nrm[:, d] * F(1.0)).astype(F)
                c = np.zeros((n, NC), F)
                if b["gk"] == GRAD_NEAREST:
                    c[:, 0] = F(-1.0) * cw
                    c[:, 1 << d] = F(1.0) * cw
                    rhs = (gd * cw).astype(F)
                else:
                    term = F(F(cw * F(2.0)) / F(NC))
                    for q in range(NC):
                        c[:, q] = (F(1.0) if (q >> d) & 1 else F(-1.0)) * term
                    rhs = (cw * gd).astype(F)
                rows.append((emitted, cell, c, rhs))
    return rows


def residuals(sizes, batches, field, dtype=np.float32, rounded=True):
    """r of every data point against `field` (x fastest): float32; -1 for a point that emits no row.  dtype: the context's
    precision (float64: coefficients and rhs formed in float32, then widened; rounded=False keeps r in that precision)."""
    T = np.dtype(dtype).type
    gn = np.asarray(sizes, np.int64)
    D = len(gn)
    NC = 1 << D
    stride = np.concatenate([[1], np.cumprod(gn[:-1])]).astype(np.int64)
    x = np.asarray(field).reshape(-1).astype(T)
    out = []
    for b in batches:
        if b["prior"] or len(b["pos"]) == 0:
            continue
        n = len(b["pos"])
        ss = np.zeros(n, T)
        has = np.zeros(n, bool)
        with np.errstate(invalid="ignore", over="ignore"):
            for emitted, origin, c, rhs in _point_rows(sizes, b):
                e = np.zeros(n, T)
                for q in range(NC):
                    cc = origin + ((q >> np.arange(D)) & 1)
                    inside = ((0 <= cc) & (cc < gn)).all(axis=1)
                    idx = (np.clip(cc, 0, gn - 1) * stride).sum(axis=1)
                    term = (c[:, q].astype(T) * x[idx]).astype(T)
                    e = np.where(inside, (e + term).astype(T), e)
                e = (e - rhs.astype(T)).astype(T)
                ss = np.where(emitted, (ss + (e * e).astype(T)).astype(T), ss)
                has |= emitted
            r = np.sqrt(ss)
        R_ = F if rounded else T
        out.append(np.where(has, r.astype(R_), R_(-1.0)).astype(R_))
    return np.concatenate(out) if out else np.zeros(0, F if rounded else T)


def scale(r):
    """s = 1.4826f x the element of rank (M - 1) // 2 of the residuals >= 0 in ascending order; 0 without any."""
    r = np.asarray(r, F)
    live = np.sort(r[r >= 0])
    if len(live) == 0:
        return F(0.0)
    return F(F(1.4826) * live[(len(live) - 1) // 2])


def omega(loss, r, s, tuning=0.0):
    """The weight factors, all in float32; None when s == 0 (the step changes nothing)."""
    r = np.asarray(r, F)
    s = F(s)
    if s == 0:
        return None
    c = F(tuning) if tuning > 0 else DEFAULT_TUNING[loss]
    sc = F(s * c)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = (r / sc).astype(F)
        if loss == HUBER:
            w = np.where(u <= 1, F(1.0), (F(1.0) / u).astype(F))
        elif loss == CAUCHY:
            w = (F(1.0) / (F(1.0) + (u * u).astype(F)).astype(F)).astype(F)
        elif loss == TUKEY:
            t = (F(1.0) - (u * u).astype(F)).astype(F)
            w = np.where(u < 1, (t * t).astype(F), F(0.0))
        else:
            raise ValueError(loss)
    return np.where(r < 0, F(1.0), w).astype(F)


def base_weights(batches):
    return np.concatenate([np.ones(len(b["pos"]), F) if b["pw"] is None else b["pw"] for b in batches if not b["prior"]])


def point_weights(base, om):
    """pw = base * sqrtf(omega) in float32"""
    return (np.asarray(base, F) * np.sqrt(np.asarray(om, F))).astype(F)


def with_weights(batches, pw):
    """the same batches carrying the point weights pw (in point order)"""
    out, off = [], 0
    for b in batches:
        nb = dict(b)
        if not b["prior"]:
            nb["pw"] = np.ascontiguousarray(pw[off:off + len(b["pos"])], F)
            off += len(b["pos"])
        out.append(nb)
    return out


def oracle_field(sizes, weights, batches):
    """The oracle's field of the batches: value data through add_value_constraints, oriented points through add_points."""
    from oracle import fi_oracle
    f = fi_oracle.LatticeField(sizes)
    f.add_field_constraints(weights)
    for b in batches:
        if b["nrm"] is None:
            if b["vk"] != VALUE_LINEAR:
                raise ValueError("value data without normals take the linear value kernel")
            f.add_value_constraints(b["pos"], np.zeros(len(b["pos"]), F) if b["val"] is None else b["val"], float(b["vw"]), b["pw"])
        else:
            if b["val"] is not None and np.any(b["val"] != 0):
                raise ValueError("the oracle's add_points has no values")
            f.add_points(float(b["vw"]), b["vk"], float(b["gw"]), b["gk"], b["pos"], b["nrm"], b["pw"])
    return f


def irls(sizes, weights, batches, loss=HUBER, tuning=0.0, rounds=5, user_scale=0.0, first=None):
    """The reference loop in fp64: an exact solve (or `first`, its result from an earlier call), then `rounds` times residuals
    (fp64) -> scale -> omega -> an oracle field with the point weights base * sqrt(omega), solved exactly.
    -> (field float64, omega float32, [field of every solve])"""
    x = oracle_field(sizes, weights, batches).solve_exact_f64() if first is None else first
    base = base_weights(batches)
    om = np.ones(len(base), F)
    fields = [x]
    for _ in range(rounds):
        r = residuals(sizes, batches, x, np.float64)
        s = F(user_scale) if user_scale > 0 else scale(r)
        new = omega(loss, r, s, tuning)
        if new is None:
            break
        om = new
        x = oracle_field(sizes, weights, with_weights(batches, point_weights(base, om))).solve_exact_f64()
        fields.append(x)
    return x, om, fields


# ---- the noisy value data of the tests: a smooth truth, N(0, 0.05) noise on every value, 10 % of them shifted by +-U(1, 3)
def truth(sizes, coords):
    """0.5 sin(5u) cos(4v) cos(3w), u, v, w = the lattice coordinates scaled to [0, 1]"""
    c = np.asarray(coords, np.float64) / (np.asarray(sizes, np.float64) - 1.0)
    k = (5.0, 4.0, 3.0)
    out = 0.5 * np.sin(k[0] * c[..., 0])
    for d in range(1, len(sizes)):
        out = out * np.cos(k[d] * c[..., d])
    return out


def truth_on_lattice(sizes):
    grids = np.meshgrid(*[np.arange(n) for n in sizes], indexing="ij")      # axis 0 = x ... ; x fastest below
    coords = np.stack(grids, axis=-1).astype(np.float64)
    return truth(sizes, coords).transpose(*reversed(range(len(sizes)))).reshape(-1)


def noisy_value_data(sizes, npoints, seed):
    """-> (batch of value points, mask of the shifted ones)"""
    rng = np.random.default_rng(seed)
    D = len(sizes)
    pos = (rng.random((npoints, D)) * (np.asarray(sizes) - 1.0)).astype(F)
    val = truth(sizes, pos.astype(np.float64)) + rng.normal(0.0, 0.05, npoints)
    bad = rng.random(npoints) < 0.10
    shift = rng.uniform(1.0, 3.0, npoints) * np.where(rng.random(npoints) < 0.5, -1.0, 1.0)
    val = np.where(bad, val + shift, val)
    return batch(pos, val=val, vw=1.0, vk=VALUE_LINEAR), bad


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
