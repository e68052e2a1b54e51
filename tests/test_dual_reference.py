"""The numpy oracle of the dual-contouring contract (tests/dual_reference.py) against the reference's own compiled
dc::dual_contouring_2d (tests/golden/dual_contouring_2d_ref.npz, recorded as tests/golden/dual_contouring_2d_ref.md says):
vertices and segments bit for bit.  In 3-D, where the reference has no counterpart, the oracle's meshes must be closed and
oriented.  CPU only."""
import os

import numpy as np
import pytest

import dual_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dual_contouring_2d_ref.npz")


def fixture_cases():
    z = np.load(GOLDEN)
    out = []
    for i, name in enumerate(z["names"]):
        p = "c%d_" % i
        g = z[p + "gradients"]
        out.append(dict(name=str(name), field=z[p + "field"], sizes=[int(s) for s in z[p + "sizes"]], iso=float(z[p + "iso"]),
                        gradients=None if len(g) == 0 else g, vertices=z[p + "vertices"], segments=z[p + "segments"]))
    return out


CASES = fixture_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_oracle_equals_the_reference(case):
    v, n, idx, keys, solves, fallback = R.contour(case["field"], case["sizes"], case["iso"], case["gradients"])
    # parity holds where the reference's loop ends finite within 32 solves: every fixture cell does
    assert len(solves) and solves.max() <= R.MAX_SOLVES and not fallback.any()
    assert v.shape == case["vertices"].shape
    assert np.array_equal(v.view(np.uint32), case["vertices"].view(np.uint32))
    assert np.array_equal(idx, case["segments"])
    assert np.all(np.diff(keys) > 0)


def test_fixture_covers_the_cases_the_contract_names():
    names = [c["name"] for c in CASES]
    assert len(names) == 8
    z = {c["name"]: c for c in CASES}
    assert (z["exact_zeros"]["field"] == 0).sum() > 0      # lattice points exactly on the contour
    assert z["iso_nonzero"]["iso"] != 0
    assert sum(c["gradients"] is not None and c["sizes"][0] != c["sizes"][1] for c in CASES) == 2
    assert z["config3_sample"]["sizes"] == [128, 128]


def left_inside_2d(f, sizes, v, idx):
    """every segment has the inside (d <= 0) on its left: the field just left of its midpoint is below the field just right"""
    a, b = v[idx[:, 0]].astype(np.float64), v[idx[:, 1]].astype(np.float64)
    t = b - a
    left = np.stack([-t[:, 1], t[:, 0]], 1)
    mid = 0.5 * (a + b)
    F = np.asarray(f, np.float64).reshape(sizes[1], sizes[0])

    def bilinear(p):
        c = np.clip(np.floor(p).astype(int), 0, np.array(sizes) - 2)
        u = p - c
        x0, y0 = c[:, 0], c[:, 1]
        return ((1 - u[:, 0]) * (1 - u[:, 1]) * F[y0, x0] + u[:, 0] * (1 - u[:, 1]) * F[y0, x0 + 1]
                + (1 - u[:, 0]) * u[:, 1] * F[y0 + 1, x0] + u[:, 0] * u[:, 1] * F[y0 + 1, x0 + 1])
    return bilinear(mid + 0.05 * left) < bilinear(mid - 0.05 * left)


def inside_on_the_left(d, sizes, keys, idx):
    """per segment: the lattice edge it crosses (the one its two cells share) has its inside end (d <= 0) on the left of the
    step from the first cell's centre to the second's"""
    nx = sizes[0]
    ca = np.stack([keys[idx[:, 0]] % nx, keys[idx[:, 0]] // nx], 1)
    cb = np.stack([keys[idx[:, 1]] % nx, keys[idx[:, 1]] // nx], 1)
    step = cb - ca
    assert (np.abs(step).sum(axis=1) == 1).all()
    left = np.stack([-step[:, 1], step[:, 0]], 1)
    p = np.maximum(ca, cb)                # the shared edge runs from p along the axis the step does not take
    end = p + (left > 0)                  # its end on the left of the step
    dd = np.asarray(d, np.float32).reshape(-1)
    return dd[end[:, 0] + nx * end[:, 1]] <= 0


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_2d_inside_on_the_left(case):
    v, n, idx, keys, solves, fb = R.contour(case["field"], case["sizes"], case["iso"], case["gradients"])
    assert inside_on_the_left(R.distances(case["field"], case["iso"]), case["sizes"], keys, idx).all()


def test_2d_circle_inside_on_the_left():
    c = CASES[0]
    v, n, idx, keys, solves, fb = R.contour(c["field"], c["sizes"])
    assert left_inside_2d(c["field"], c["sizes"], v, idx).all()
    # one closed loop: every vertex starts one segment and ends one
    assert np.array_equal(np.sort(idx[:, 0]), np.arange(len(v))) and np.array_equal(np.sort(idx[:, 1]), np.arange(len(v)))
    # normals point away from the centre
    centre = np.array([19.3, 18.7])
    assert (np.sum(n * (v - centre), axis=1) > 0).all()


def sphere(sizes, c, r):
    g = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sizes[::-1]], indexing="ij")
    d2 = sum((g[len(sizes) - 1 - k] - c[k]) ** 2 for k in range(len(sizes)))
    return (np.sqrt(d2) - r).astype(np.float32).reshape(-1)


def box(sizes, c, h):
    g = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sizes[::-1]], indexing="ij")
    q = [np.abs(g[len(sizes) - 1 - k] - c[k]) - h[k] for k in range(len(sizes))]
    out = np.sqrt(sum(np.maximum(x, 0) ** 2 for x in q)) + np.minimum(np.maximum.reduce(q), 0)
    return out.astype(np.float32).reshape(-1)


def closed_oriented(idx):
    """every undirected edge in exactly two triangles, once in each direction"""
    e = np.concatenate([idx[:, [0, 1]], idx[:, [1, 2]], idx[:, [2, 0]]])
    directed = {tuple(x) for x in e.tolist()}
    if len(directed) != len(e):
        return False
    return all((b, a) in directed for a, b in directed)


def boundary_free(idx):
    """as a chain the mesh has no boundary: each directed edge occurs as often as its reverse (a cell of an ambiguous case
    has one vertex for several sheets, so an edge may belong to four triangles)"""
    from collections import Counter
    e = Counter(map(tuple, np.concatenate([idx[:, [0, 1]], idx[:, [1, 2]], idx[:, [2, 0]]]).tolist()))
    return all(e[(b, a)] == k for (a, b), k in e.items())


def signed_volume(v, idx):
    a, b, c = (v[idx[:, k]].astype(np.float64) for k in range(3))
    return np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0


@pytest.mark.parametrize("sizes,c,r", [([20, 18, 17], (9.3, 8.6, 8.2), 5.7), ([16, 16, 16], (7.5, 7.5, 7.5), 4.0),
                                       ([24, 22, 21], (11.1, 10.4, 10.3), 8.2)])
def test_3d_sphere_closed_and_oriented(sizes, c, r):
    f = sphere(sizes, c, r)
    v, n, idx, keys, solves, fb = R.contour(f, sizes)
    assert idx.shape[1] == 3 and closed_oriented(idx)
    vol = signed_volume(v, idx)
    assert abs(vol - 4.0 / 3.0 * np.pi * r ** 3) <= 0.03 * 4.0 / 3.0 * np.pi * r ** 3
    # normals: outwards
    assert (np.sum(n * (v - np.array(c)), axis=1) > 0).all()


def test_3d_box_with_analytic_gradients_keeps_its_corners():
    sizes, c, h = [22, 21, 20], np.array([10.37, 10.21, 9.63]), np.array([5.3, 4.6, 4.15])
    f = box(sizes, c, h)
    v, n, idx, keys, solves, fb = R.contour(f, sizes, 0.0, box_gradients(sizes, c, h))
    assert closed_oriented(idx) and signed_volume(v, idx) > 0
    corners = np.array([[c[k] + s[k] * h[k] for k in range(3)] for s in np.array(np.meshgrid([-1, 1], [-1, 1], [-1, 1])).T.reshape(-1, 3)])
    dist = np.min(np.linalg.norm(v[None, :, :] - corners[:, None, :], axis=2), axis=1)
    assert dist.max() <= 0.01


def box_gradients(sizes, c, h):
    """the gradient of the exact box SDF (outside: towards the nearest box point; inside: the axis of the nearest face)"""
    g = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sizes[::-1]], indexing="ij")
    p = np.stack([g[2 - k].reshape(-1) for k in range(3)], 1) - c
    q = np.abs(p) - h
    outside = np.maximum(q, 0)
    ln = np.linalg.norm(outside, axis=1)
    gr = np.where(ln[:, None] > 0, np.sign(p) * outside / np.maximum(ln, 1e-30)[:, None], 0.0)
    k = np.argmax(q, axis=1)
    inner = np.zeros_like(p)
    inner[np.arange(len(p)), k] = np.sign(p[np.arange(len(p)), k])
    gr = np.where((ln > 0)[:, None], gr, inner)
    return gr.astype(np.float32)


def test_random_3d_field_has_no_boundary_where_the_lattice_closes_it():
    rng = np.random.default_rng(1)
    sizes = [12, 11, 10]
    f = rng.normal(size=int(np.prod(sizes))).astype(np.float32)
    # pad with an outside border so every crossing edge has its four cells
    F = np.full((sizes[2] + 4, sizes[1] + 4, sizes[0] + 4), 1.0, np.float32)
    F[2:-2, 2:-2, 2:-2] = f.reshape(sizes[::-1])
    v, n, idx, keys, solves, fb = R.contour(F.reshape(-1), [s + 4 for s in sizes])
    assert boundary_free(idx) and signed_volume(v, idx) > 0


def test_conventions():
    with pytest.raises(R.Unsupported):
        R.contour(np.zeros(5, np.float32), [5])
    f = np.ones(16, np.float32)
    f[5] = np.nan
    with pytest.raises(R.NonFinite):
        R.contour(f, [4, 4])
    assert len(R.contour(np.full(5, np.nan, np.float32), [1, 5])[0]) == 0   # no cell: nothing read
    v = R.contour(np.array([0.0, 1.0, 1.0, 1.0], np.float32), [2, 2])[0]     # d = 0 is inside
    assert len(v) == 1
