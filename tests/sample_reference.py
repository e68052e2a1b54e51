"""Numpy oracle of the point-query contract (include/fi_hip.h fi_sample): every product and sum in the
contract's order, in `dtype` (float32: one rounding per operation, as the device kernels with -ffp-contract=off; float64: the
path of an FI_F64 context sampling its own solution, each output rounded to fp32 once).  Only numpy."""
import numpy as np


def _strides(sizes):
    s = [1]
    for n in sizes[:-1]:
        s.append(s[-1] * int(n))
    return s


def locate(sizes, positions, dtype=np.float32):
    """(inside mask, cells c (m, D) int64, offsets t (m, D) dtype) of the inside points"""
    D = len(sizes)
    p = np.asarray(positions, np.float32).reshape(-1, D)
    hi = np.array([n - 1 for n in sizes], np.float32)
    with np.errstate(invalid="ignore"):
        inside = np.all(np.isfinite(p) & (p >= np.float32(0)) & (p <= hi), axis=1)
    pi = p[inside]
    c = np.minimum(np.floor(pi).astype(np.int64), np.array(sizes, np.int64) - 2)
    t = pi.astype(dtype) - c.astype(dtype)
    return inside, c, t


def linear_weights(t):
    """w_i = u_0(b_0) * u_1(b_1) * u_2(b_2), left to right, for corners i = 0 .. 2^D - 1 (bit d: +1 along axis d)"""
    T = t.dtype.type
    D = t.shape[1]
    u = [(T(1) - t[:, d], t[:, d]) for d in range(D)]
    out = []
    for i in range(1 << D):
        w = u[0][i & 1]
        for d in range(1, D):
            w = w * u[d][(i >> d) & 1]
        out.append(w)
    return out, u


def _catmull_rom(p0, p1, p2, p3):
    T = p0.dtype.type
    a = p2 - p0
    b = ((T(2) * p0 - T(5) * p1) + T(4) * p2) - p3
    e = (T(3) * (p1 - p2) + p3) - p0
    return p1, a, b, e


def _cr_val(k, t):
    p1, a, b, e = k
    T = t.dtype.type
    return p1 + (T(0.5) * t) * (a + t * (b + t * e))


def _cr_der(k, t):
    _, a, b, e = k
    T = t.dtype.type
    return T(0.5) * (a + t * (T(2) * b + (T(3) * t) * e))


def _linear(f, sizes, c, t, grads):
    D = len(sizes)
    s = _strides(sizes)
    base = sum(s[d] * c[:, d] for d in range(D))
    fv = [f[base + sum(s[d] for d in range(D) if (i >> d) & 1)] for i in range(1 << D)]
    w, u = linear_weights(t)
    v = None
    for i in range(1 << D):
        term = w[i] * fv[i]
        v = term if v is None else v + term
    g = []
    if grads:
        for d in range(D):
            acc = None
            for i in range(1 << D):
                if (i >> d) & 1:
                    continue
                term = fv[i | (1 << d)] - fv[i]
                if D > 1:
                    W = None
                    for e in range(D):
                        if e != d:
                            W = u[e][(i >> e) & 1] if W is None else W * u[e][(i >> e) & 1]
                    term = W * term
                acc = term if acc is None else acc + term
            g.append(acc)
    return v, g


def _cubic(f, sizes, c, t, grads):
    D = len(sizes)
    s = _strides(sizes)
    idx = [[s[d] * np.clip(c[:, d] - 1 + k, 0, sizes[d] - 1) for k in range(4)] for d in range(D)]
    tx = t[:, 0]
    if D == 1:
        kx = _catmull_rom(*[f[idx[0][k]] for k in range(4)])
        return _cr_val(kx, tx), ([_cr_der(kx, tx)] if grads else [])

    def plane(oz):
        r, dr = [], []
        for j in range(4):
            kx = _catmull_rom(*[f[oz + idx[1][j] + idx[0][k]] for k in range(4)])
            r.append(_cr_val(kx, tx))
            dr.append(_cr_der(kx, tx))
        ty = t[:, 1]
        ky = _catmull_rom(*r)
        return _cr_val(ky, ty), _cr_val(_catmull_rom(*dr), ty), _cr_der(ky, ty)

    if D == 2:
        v, gx, gy = plane(0)
        return v, ([gx, gy] if grads else [])
    P, GX, GY = zip(*[plane(idx[2][m]) for m in range(4)])
    tz = t[:, 2]
    kz = _catmull_rom(*P)
    v = _cr_val(kz, tz)
    if not grads:
        return v, []
    return v, [_cr_val(_catmull_rom(*GX), tz), _cr_val(_catmull_rom(*GY), tz), _cr_der(kz, tz)]


def sample(field, sizes, positions, cubic=False, gradients=False, fill=np.nan, dtype=np.float32):
    """values (n,) float32, and with gradients=True also (n, D) float32, of `field` (flat, x fastest) at `positions`"""
    sizes = [int(n) for n in sizes]
    D = len(sizes)
    f = np.asarray(field).reshape(-1).astype(dtype)
    inside, c, t = locate(sizes, positions, dtype)
    n = len(inside)
    vals = np.full(n, np.float32(fill), np.float32)
    grads = np.full((n, D), np.float32(fill), np.float32)
    if inside.any():
        with np.errstate(invalid="ignore", over="ignore"):
            v, g = (_cubic if cubic else _linear)(f, sizes, c, t, gradients)
        vals[inside] = v.astype(np.float32)
        for d, gd in enumerate(g):
            grads[inside, d] = gd.astype(np.float32)
    return (vals, grads) if gradients else vals
