"""Meshes, fields and rays shared by the ray tests (tests/test_ray_reference.py, tests/test_gpu_ray.py): only numpy."""
import numpy as np

import surface_reference as S
from nearest_reference import lattice_points

F = np.float32

# the unit cube on integer vertices (vertex x + 2 y + 4 z), two triangles per face, outward or not: the contract does not care
CUBE_V = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], F)
CUBE_I = np.array([[0, 2, 3], [0, 3, 1],      # z = 0
                   [4, 5, 7], [4, 7, 6],      # z = 1
                   [0, 1, 5], [0, 5, 4],      # y = 0
                   [2, 6, 7], [2, 7, 3],      # y = 1
                   [0, 4, 6], [0, 6, 2],      # x = 0
                   [1, 3, 7], [1, 7, 5]], np.int32)
SQUARE_V = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F)
SQUARE_I = np.array([[0, 1], [1, 2], [2, 3], [3, 0]], np.int32)

BLOB_SIZES = [12, 11, 10]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert bad.size == 0, (bad[:10], got.reshape(-1)[bad[:10]], want.reshape(-1)[bad[:10]])


def blob(sizes=BLOB_SIZES):
    """the closed blob: |p - c| - 3.7 + 0.4 cos(1.3 x + 0.7 y) sin(0.9 z) (2-D: without the sine)"""
    p = lattice_points(sizes).astype(np.float64)
    c = np.array([5.3, 5.1, 4.6])[:len(sizes)]
    w = np.cos(1.3 * p[:, 0] + 0.7 * p[:, 1])
    if len(sizes) == 3:
        w = w * np.sin(0.9 * p[:, 2])
    return (np.linalg.norm(p - c, axis=1) - 3.7 + 0.4 * w).astype(F)


def closed_field(sizes):
    """a wobbly ball well inside the lattice of `sizes`: its iso-0 mesh is closed"""
    p = lattice_points(sizes).astype(np.float64)
    n = np.array(sizes, np.float64)
    c = (n - 1) / 2 + np.array([0.3, -0.4, 0.1])[:len(sizes)]
    r = 0.33 * (n.min() - 1)
    w = np.cos(0.9 * p[:, 0] + 0.4 * p[:, 1])
    if len(sizes) == 3:
        w = w * np.sin(0.7 * p[:, 2] + 0.2)
    return (np.linalg.norm(p - c, axis=1) - r + 0.07 * r * w).astype(F)


def smooth(sizes, seed, waves=5, k=0.3):
    """tests/test_gpu_surface.py's smooth field"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sizes[::-1]], indexing="ij")
    f = np.zeros(g[0].shape)
    for _ in range(waves):
        kk = rng.normal(size=len(sizes)) * k
        f += np.cos(sum(a * b for a, b in zip(kk[::-1], g)) + rng.uniform(0, 6.3))
    return f.astype(F).reshape(-1)


_MESHES = {}


def mesh_of(kind, sizes, method):
    """(vertices, indices, inside mask, field, iso) of a field's mesh, computed once: kind 'blob' or 'closed' (iso 0) or 'smooth'
    (seed sum(sizes), iso its median)"""
    key = (kind, tuple(sizes), method)
    if key not in _MESHES:
        f = blob(sizes) if kind == "blob" else closed_field(sizes) if kind == "closed" else smooth(sizes, sum(sizes))
        iso = float(np.median(f)) if kind == "smooth" else 0.0
        v, i, inside = S.surface(f, sizes, iso, method)
        v = np.ascontiguousarray(v, F).reshape(-1, len(sizes))
        i = np.ascontiguousarray(i, np.int32).reshape(-1, len(sizes))
        for a in (v, i, inside, f):
            a.setflags(write=False)
        _MESHES[key] = (v, i, inside, f, iso)
    return _MESHES[key]


def axis_directions(ndim):
    d = np.zeros((2 * ndim, ndim), F)
    for a in range(ndim):
        d[2 * a, a], d[2 * a + 1, a] = 1, -1
    return d


def soup(n, seed, ndim=3, shift=0.0, flat=False, bad=False):
    """n random primitives in [0, 10)^ndim + shift; flat: every third one axis-aligned (a flat box); bad: some vertices
    non-finite"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 10, (n, 1, ndim))
    P = (c + rng.normal(size=(n, ndim, ndim)) * 0.8).astype(F)
    if flat:
        for j in range(0, n, 3):
            P[j, :, j % ndim] = P[j, 0, j % ndim]
        P = np.round(P * 4) / 4                      # quarter-unit vertices: rays through vertices and edges happen
    P = (P + F(shift)).astype(F)
    V = P.reshape(-1, ndim).copy()
    if bad:
        V[rng.choice(V.shape[0], max(1, n // 10), replace=False), 0] = [np.nan, np.inf][n % 2]
    return V, np.arange(n * ndim, dtype=np.int32).reshape(n, ndim)


def soup_rays(n, seed, ndim=3, shift=0.0, flat=False):
    """rays at a soup: random ones, axis-parallel ones and, for flat soups, ones on the quarter-unit grid"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-3, 13, (n, ndim))
    d = (rng.uniform(0, 10, (n, ndim)) - o) * rng.uniform(0.05, 0.5, (n, 1))   # towards the soup
    ax = rng.integers(0, ndim, n)
    par = rng.random(n) < 0.3
    d[par] = 0
    d[par, ax[par]] = rng.choice([-2.0, 1.0, 0.5], par.sum())
    if flat:
        o = np.round(o * 4) / 4
        d = np.where(par[:, None], d, np.round(d * 2) / 2)
    return (o + shift).astype(F), d.astype(F)


def aim(o, d, v, i, seed):
    """every second ray of (o, d) turned towards a point of a primitive of the mesh (v, i): a vertex for every eighth ray
    (in float32 the ray then passes through it or next to it), else a random point of the primitive"""
    rng = np.random.default_rng(seed)
    n, ndim = o.shape
    o, d = o.copy(), d.copy()
    if n == 0 or len(i) == 0:
        return o, d
    w = rng.dirichlet(np.ones(ndim), n)
    w[::8] = np.eye(ndim)[rng.integers(0, ndim, len(w[::8]))]
    target = np.einsum("nk,nkd->nd", w, v[i[rng.integers(0, len(i), n)]].astype(np.float64))
    d[::2] = ((target - o) * rng.choice([0.25, 0.5, 1.0], (n, 1)))[::2]
    return o, d.astype(F)
