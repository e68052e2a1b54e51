"""The contract of the march unit (include/fi_hip.h fi_field_raycast, fi_field_render) restated in numpy: fp32
elementwise, one rounding per operation, written for all rays at once (a loop over the samples, the rays that are still
marching in step).  The device is held to these functions bit for bit (tests/test_gpu_march.py);
tests/test_march_reference.py holds them to geometry known by hand.  Values and gradients are sample_reference.sample's.
Only numpy."""
import numpy as np

import depth_reference
import sample_reference

F = np.float32
FRONT, BACK, EITHER = 0, 1, 2
MAX_SAMPLES = 1 << 20          # FI_MARCH_MAX_SAMPLES
INF = F(np.inf)


def _min(a, b):
    return np.where(a < b, a, b)


def _max(a, b):
    return np.where(a > b, a, b)


def _length(d):
    l2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    if d.shape[1] == 3:
        l2 = l2 + d[:, 2] * d[:, 2]
    return np.sqrt(l2)


class _Field:
    def __init__(self, field, sizes, weight, min_weight):
        self.sizes = [int(n) for n in sizes]
        self.D = len(self.sizes)
        self.f = np.asarray(field, F).reshape(-1)
        assert self.D in (2, 3) and min(self.sizes) >= 2 and self.f.size == int(np.prod(self.sizes))
        self.hi = np.array([n - 1 for n in self.sizes], F)
        self.cell_ok = None
        if weight is not None:
            w = np.asarray(weight, F).reshape(self.sizes[::-1])
            with np.errstate(invalid="ignore"):
                ok = (w > 0) & (w >= F(min_weight))
            cells = ok[tuple(slice(0, -1) for _ in range(self.D))].copy()
            for corner in range(1, 1 << self.D):           # axis D - 1 - j of the array is lattice axis j
                cells &= ok[tuple(slice(1, None) if (corner >> (self.D - 1 - a)) & 1 else slice(0, -1) for a in range(self.D))]
            self.cell_ok = cells

    def positions(self, o, d, t):
        """step 3: the sample positions at t, inside the box"""
        p = o + t[:, None] * d
        return np.where(p > 0, np.where(p > self.hi, self.hi, p), F(0)).astype(F)

    def sample(self, p, gradients=False):
        """(values, valid[, gradients]) at positions inside the box"""
        out = sample_reference.sample(self.f, self.sizes, p, gradients=gradients)
        v, g = out if gradients else (out, None)
        valid = np.isfinite(v)
        if self.cell_ok is not None:
            c = np.minimum(np.floor(p).astype(np.int64), np.array(self.sizes, np.int64) - 2)
            valid &= self.cell_ok[tuple(c[:, j] for j in range(self.D - 1, -1, -1))]
        return (v, valid, g) if gradients else (v, valid)


def raycast(field, sizes, origins, directions, iso=0.0, step=1.0, refine=4, side=FRONT, weight=None, min_weight=0.0, t_min=0.0,
            t_max=np.inf):
    """fi_field_raycast -> t (n,), positions (n, D), normals (n, D) float32, side (n,) int8"""
    fld = _Field(field, sizes, weight, min_weight)
    D = fld.D
    o = np.asarray(origins, F).reshape(-1, D)
    d = np.asarray(directions, F).reshape(-1, D)
    n = len(o)
    iso, step, t_min, t_max = F(iso), F(step), F(t_min), F(t_max)
    t = np.full(n, F(np.nan), F)
    pos = np.full((n, D), F(np.nan), F)
    nrm = np.zeros((n, D), F)
    sd = np.zeros(n, np.int8)
    with np.errstate(all="ignore"):
        ln = _length(d)
        ray = np.all(np.isfinite(o) & np.isfinite(d), axis=1) & (ln > 0) & (ln < INF)
        t[ray] = INF
        te, tx, miss = np.full(n, -INF, F), np.full(n, INF, F), np.zeros(n, bool)
        for j in range(D):
            par = d[:, j] == 0
            miss |= par & ~((o[:, j] >= 0) & (o[:, j] <= fld.hi[j]))
            u, v = (F(0) - o[:, j]) / d[:, j], (fld.hi[j] - o[:, j]) / d[:, j]
            te = np.where(par, te, _max(te, _min(u, v)))
            tx = np.where(par, tx, _min(tx, _max(u, v)))
        ta, tb = _max(te, t_min), _min(tx, t_max)
        dt = step / ln
        go = ray & ~miss & ~(ta > tb) & np.isfinite(ta) & np.isfinite(tb) & (dt > 0) & (dt < INF)

        idx = np.nonzero(go)[0]                 # the rays still marching
        o_, d_, ta_, tb_, dt_ = o[idx], d[idx], ta[idx], tb[idx], dt[idx]
        pt, pf, pv = np.zeros(len(idx), F), np.zeros(len(idx), F), np.zeros(len(idx), bool)
        hit_i, hit_a, hit_b, hit_fa, hit_fb, hit_s = [], [], [], [], [], []
        for k in range(MAX_SAMPLES):
            if len(idx) == 0:
                break
            raw = ta_ + F(k) * dt_
            tk = _min(raw, tb_)
            f, v = fld.sample(fld.positions(o_, d_, tk))
            both = pv & v
            ip, ic = pf < iso, f < iso
            s = np.zeros(len(idx), np.int8)
            if side != BACK:
                s[both & ~ip & ic] = 1
            if side != FRONT:
                s[both & ip & ~ic] = -1
            h = s != 0
            hit_i.append(idx[h]), hit_a.append(pt[h]), hit_b.append(tk[h]), hit_fa.append(pf[h]), hit_fb.append(f[h]), hit_s.append(s[h])
            keep = ~h & (raw < tb_)
            idx, o_, d_, ta_, tb_, dt_ = idx[keep], o_[keep], d_[keep], ta_[keep], tb_[keep], dt_[keep]
            pt, pf, pv = tk[keep], f[keep], v[keep]
        if hit_i:
            hi_ = np.concatenate(hit_i)
            a, b, fa, fb, hs = (np.concatenate(x) for x in (hit_a, hit_b, hit_fa, hit_fb, hit_s))
            oh, dh = o[hi_], d[hi_]
            live = np.ones(len(hi_), bool)
            for _ in range(int(refine)):
                m = F(0.5) * (a + b)
                f, v = fld.sample(fld.positions(oh, dh, m))
                live &= v
                same = (f < iso) == (fa < iso)
                a, fa = np.where(live & same, m, a), np.where(live & same, f, fa)
                b, fb = np.where(live & ~same, m, b), np.where(live & ~same, f, fb)
            th = (a + ((fa - iso) / (fa - fb)) * (b - a)).astype(F)
            p = fld.positions(oh, dh, th)
            _, _, g = fld.sample(p, gradients=True)
            l2 = g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]
            if D == 3:
                l2 = l2 + g[:, 2] * g[:, 2]
            gl = np.sqrt(l2)
            good = (gl > 0) & (gl < INF)
            t[hi_], pos[hi_], sd[hi_] = th, p, hs
            nrm[hi_] = np.where(good[:, None], g / gl[:, None], F(0))
    return t, pos, nrm, sd


def pixel_rays(cam):
    """the rays of an fi_camera's pixels in pixel order: origins (h w, 3), directions (h w, 3), px, py (h w,)"""
    rows, cols = np.meshgrid(np.arange(cam.height), np.arange(cam.width), indexing="ij")
    rows, cols = rows.reshape(-1), cols.reshape(-1)
    px = ((cols.astype(F) + F(0.5)) - cam.cx) / cam.fx
    py = ((rows.astype(F) + F(0.5)) - cam.cy) / cam.fy
    R, e = cam.pose[:, :3], F(0) - cam.pose[:, 3]
    o = np.stack([np.full(len(px), (R[0, j] * e[0] + R[1, j] * e[1]) + R[2, j] * e[2], F) for j in range(3)], axis=1)
    d = np.stack([(R[0, j] * px + R[1, j] * py) + R[2, j] for j in range(3)], axis=1).astype(F)
    return o, d, px, py


def render(field, sizes, cam, iso=0.0, step=1.0, refine=4, side=FRONT, weight=None, min_weight=0.0):
    """fi_field_render -> depth (h w,), positions (h w, 3), normals (h w, 3), incidence (h w,) float32"""
    o, d, px, py = pixel_rays(cam)
    t, pos, nrm, sd = raycast(field, sizes, o, d, iso, step, refine, side, weight, min_weight, 0.0, np.inf)
    hit = sd != 0
    with np.errstate(all="ignore"):
        scale = F(1) if cam.kind == depth_reference.Z else np.sqrt((px * px + py * py) + F(1))
        depth = np.where(hit, t * scale, INF).astype(F)
        ln = _length(d)
        s = (nrm[:, 0] * (d[:, 0] / ln) + nrm[:, 1] * (d[:, 1] / ln)) + nrm[:, 2] * (d[:, 2] / ln)
        q = -s
        q = np.where(q < 1, q, F(1))
        lit = hit & (q > 0)
    return depth, pos, np.where(lit[:, None], nrm, F(0)).astype(F), np.where(lit, q, F(0)).astype(F)


def _rigid(cam):
    G = np.eye(4)
    G[:3] = cam.pose.astype(np.float64)
    return G


def track(tsdf, weight, sizes, truncation, cam, depth, register, rounds=2, max_jump=np.inf, max_distance=None, step=1.0, refine=4,
          min_weight=0.0, **keywords):
    """DepthVolume.track on the restatements: `register(source, target, target_normals, mode=, max_distance=, **keywords)`
    returns a dict with the 4 x 4 float64 "transform" -> (camera, correction (4, 4) float64, per-round dicts)"""
    max_distance = float(truncation) if max_distance is None else max_distance
    total, log = np.eye(4), []
    for _ in range(int(rounds)):
        _, pos, nrm, _ = render(tsdf, sizes, cam, 0.0, step, refine, FRONT, weight, min_weight)
        hit = np.isfinite(pos[:, 0])
        src, _, _, ok = depth_reference.unproject(cam, depth, max_jump)
        src = src[ok.astype(bool)]
        r = register(src, pos[hit], nrm[hit], mode="plane", max_distance=max_distance, **keywords)
        T = np.asarray(r["transform"], np.float64).reshape(4, 4)
        G = _rigid(cam) @ np.linalg.inv(T)
        total = T @ total
        cam = depth_reference.Cam(G[:3].astype(F), cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, cam.kind)
        log.append({"rendered": int(hit.sum()), "unprojected": int(len(src)), "registration": r})
    return cam, total, log
