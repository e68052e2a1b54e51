"""The iso-contour oracle (tests/iso_reference.py) against the contract's geometric promises, without a GPU: closed,
consistently oriented loops in every cell case, watertight oriented meshes, and the area / volume of analytic shapes."""
import math

import numpy as np
import pytest

import iso_reference as R


@pytest.mark.parametrize("case", range(16))
def test_square_cases_close_and_orient(case):
    inside = R.case_inside(2, case)
    segs = R.cell_primitives(2, inside)
    n_in = sum(inside.values())
    assert (len(segs) == 0) == (n_in in (0, 4))
    for a, b in segs:
        # inside on the left of (a -> b): the inside corners nearest the segment lie left of it
        pa = _edge_mid(2, a)
        pb = _edge_mid(2, b)
        d = pb - pa
        left = np.array([-d[1], d[0]])
        mid = (pa + pb) / 2
        for c, isin in inside.items():
            side = float(np.dot(np.array(c, float) - mid, left))
            if abs(side) > 1e-9 and np.linalg.norm(np.array(c, float) - mid) < 0.75:
                assert (side > 0) == isin, (case, a, b, c)


def _edge_mid(ndim, e):
    a, offs = R.edge_corner(ndim, e)
    p = np.array(offs, float)
    p[a] += 0.5
    return p


@pytest.mark.parametrize("case", range(256))
def test_cube_cases_close_and_orient(case):
    inside = R.case_inside(3, case)
    tris = R.cell_primitives(3, inside)
    # each crossing cube edge is used by the loops; the surface inside the cube is closed against the cube's faces:
    # every directed triangle edge between two vertices either has its reverse in the cell, or lies on a cube face
    crossing = set()
    for e in range(12):
        a, offs = R.edge_corner(3, e)
        q = list(offs)
        q[a] = 1
        if inside[offs] != inside[tuple(q)]:
            crossing.add(e)
    used = {e for t in tris for e in t}
    assert used == crossing
    # orientation: the normal of every triangle points away from the inside corners (midpoint-edge geometry)
    for t in tris:
        p = [_edge_mid(3, e) for e in t]
        nrm = np.cross(p[1] - p[0], p[2] - p[0])
        if np.linalg.norm(nrm) < 1e-12:
            continue
        cen = sum(p) / 3
        score = 0.0
        for c, isin in inside.items():
            w = 1.0 / (1e-3 + np.linalg.norm(np.array(c, float) - cen) ** 4)
            score += w * float(np.dot(np.array(c, float) - cen, nrm)) * (-1 if isin else 1)
        assert score > 0, (case, t)
    # loops: the triangle edges along the loop boundary, de-duplicated against their interior diagonals, form cycles
    bnd = {}
    for t in tris:
        for i in range(3):
            bnd[(t[i], t[(i + 1) % 3])] = bnd.get((t[i], t[(i + 1) % 3]), 0) + 1
    outer = [(a, b) for (a, b) in bnd if (b, a) not in bnd]
    starts = sorted(a for a, _ in outer)
    ends = sorted(b for _, b in outer)
    assert starts == ends == sorted(used)


def _smooth_field(sizes, seed):
    rng = np.random.default_rng(seed)
    grid = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sizes[::-1]], indexing="ij")
    f = np.zeros(grid[0].shape)
    for _ in range(6):
        k = rng.normal(size=len(sizes)) * 0.35
        ph = rng.uniform(0, 2 * np.pi)
        f += np.cos(sum(kk * g for kk, g in zip(k[::-1], grid)) + ph)
    return f.astype(np.float32).reshape(-1)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_smooth_fields_give_watertight_oriented_meshes(seed):
    sizes = [14, 12, 11]
    v, n, idx, keys = R.extract(_smooth_field(sizes, seed), sizes, 0.1)
    assert len(idx) > 0
    # edges on the lattice border are open; every other edge is used twice, once in each direction
    d = R.directed_edges(idx)
    border = []
    for a, b in d:
        pa, pb = v[a], v[b]
        on = any(
            (abs(pa[k] - lim) < 1e-6 and abs(pb[k] - lim) < 1e-6) for k in range(3) for lim in (0, sizes[k] - 1))
        border.append(on)
    ds = {}
    for (a, b), on in zip(d, border):
        if not on:
            ds[(a, b)] = ds.get((a, b), 0) + 1
    assert all(c == 1 for c in ds.values())
    assert all((b, a) in ds for (a, b) in ds)
    assert np.all(np.diff(keys) > 0)


def test_circle_area():
    r, c = 25.3, (40.2, 39.7)
    sizes = [81, 80]
    y, x = np.meshgrid(np.arange(sizes[1]), np.arange(sizes[0]), indexing="ij")
    f = (np.hypot(x - c[0], y - c[1]) - r).astype(np.float32).reshape(-1)
    v, n, idx, keys = R.extract(f, sizes)
    assert R.watertight_oriented(idx)
    area = R.signed_measure(v, idx)
    assert abs(area - math.pi * r * r) < 0.01 * math.pi * r * r
    # normals point outwards (towards increasing f)
    rad = v - np.array(c, np.float32)
    assert np.all(np.einsum("ij,ij->i", rad, n) > 0)


def test_sphere_volume():
    r, c = 20.5, (24.3, 25.1, 23.7)
    sizes = [50, 50, 49]
    z, y, x = np.meshgrid(*[np.arange(s) for s in sizes[::-1]], indexing="ij")
    f = (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r).astype(np.float32).reshape(-1)
    v, n, idx, keys = R.extract(f, sizes)
    assert R.watertight_oriented(idx)
    vol = R.signed_measure(v, idx)
    assert abs(vol - 4 / 3 * math.pi * r ** 3) < 0.01 * 4 / 3 * math.pi * r ** 3
    assert R.euler_characteristic(len(v), idx) == 2


def test_degenerate_inputs():
    with pytest.raises(R.Unsupported):
        R.extract(np.zeros(5, np.float32), [5])
    f = np.zeros(27, np.float32)
    f[3] = np.nan
    with pytest.raises(R.NonFinite):
        R.extract(f, [3, 3, 3])
    v, n, idx, keys = R.extract(np.ones(27, np.float32), [3, 3, 3])
    assert len(v) == 0 and len(idx) == 0
