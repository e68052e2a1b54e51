"""The meshes the smoothing tests share (tests/test_smooth_reference.py on the CPU, tests/test_gpu_smooth.py on the device):
constructed cases with known answers and small extracted surfaces.  Only numpy and the other restatements."""
import numpy as np

import iso_reference as R
import simplify_reference as S


def polygon(n=12, radius=5.0, centre=(7.0, 6.0)):
    """a closed regular n-gon, counter-clockwise -> (vertices float32 (n, 2), segments int32 (n, 2))"""
    a = 2.0 * np.pi * np.arange(n) / n
    v = np.stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)], axis=1).astype(np.float32)
    return v, np.array([(i, (i + 1) % n) for i in range(n)], np.int32)


def flat_grid(n=6, z=3.125, h=1.0):
    """an n x n grid of vertices at height z, two triangles a square -> (vertices, triangles, boundary mask)"""
    x, y = np.meshgrid(np.arange(n) * h, np.arange(n) * h, indexing="xy")
    v = np.stack([x, y, np.full_like(x, z)], axis=2).reshape(-1, 3).astype(np.float32)
    i = (np.arange(n - 1)[None, :] + n * np.arange(n - 1)[:, None]).reshape(-1)
    t = np.concatenate([np.stack([i, i + 1, i + n + 1], axis=1), np.stack([i, i + n + 1, i + n], axis=1)]).astype(np.int32)
    ix, iy = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    rim = ((ix == 0) | (ix == n - 1) | (iy == 0) | (iy == n - 1)).reshape(-1)
    return v, t, rim


CUT_SIZES = [20, 20, 20]


def cut_sphere():
    """a sphere of radius 5.2 at (17.3, 9.6, 10.2) on 20^3: the lattice face x = 19 cuts it open -> extract()'s mesh"""
    z, y, x = np.meshgrid(*[np.arange(20, dtype=np.float64)] * 3, indexing="ij")
    f = (np.sqrt((x - 17.3) ** 2 + (y - 9.6) ** 2 + (z - 10.2) ** 2) - 5.2).astype(np.float32).reshape(-1)
    return R.extract(f, CUT_SIZES)


def staircase():
    """the 24^3 sphere field binarised to -1 / +1: its iso-surface is the voxel staircase -> (extract()'s mesh, the centre)"""
    f, centre = S.sphere_field()
    return R.extract(np.where(f < 0, -1.0, 1.0).astype(np.float32), [24, 24, 24]), np.asarray(centre, np.float64)


def radial_rms_angle(vertices, indices, centre):
    """the area-weighted rms angle (degrees) between the face normals and the radial direction at the face centres"""
    v = np.asarray(vertices, np.float64)
    a, b, c = v[indices[:, 0]], v[indices[:, 1]], v[indices[:, 2]]
    n = np.cross(b - a, c - a)
    area = np.sqrt((n * n).sum(axis=1))
    r = (a + b + c) / 3.0 - centre[None, :]
    cosine = (n * r).sum(axis=1) / np.maximum(area * np.sqrt((r * r).sum(axis=1)), 1e-300)
    angle = np.degrees(np.arccos(np.clip(cosine, -1.0, 1.0)))
    return float(np.sqrt((area * angle * angle).sum() / area.sum()))


# constructed index lists: (name, vertices, indices)
def constructed():
    rng = np.random.default_rng(11)
    v3 = lambda n: rng.uniform(0.0, 4.0, size=(n, 3)).astype(np.float32)  # noqa: E731
    fan = np.array([[1, 1, 1], [2, 1, 1], [3, 1, 1], [4, 1, 1]], np.float32)
    return [
        ("duplicated triangles", v3(5), [[0, 1, 2], [0, 1, 2], [2, 1, 3], [2, 1, 3], [3, 1, 4]]),
        ("a triangle and its reverse", v3(4), [[0, 1, 2], [2, 1, 0], [1, 3, 2]]),
        ("repeated indices", v3(5), [[0, 0, 1], [1, 2, 2], [3, 3, 3], [0, 1, 2], [2, 1, 4], [4, 2, 4]]),
        ("an edge used three times", v3(5), [[0, 1, 2], [0, 1, 3], [0, 1, 4]]),
        ("a zero-area fan", fan, [[0, 1, 2], [0, 2, 3]]),
        ("unused and isolated vertices", v3(8), [[0, 1, 2], [2, 1, 3], [5, 5, 5]]),
        ("2-d: a chain, a doubled segment, a point", rng.uniform(0, 4, size=(9, 2)).astype(np.float32),
         [[0, 1], [1, 2], [2, 3], [4, 5], [4, 5], [5, 6], [7, 7]]),
        ("2-d: a star", rng.uniform(0, 4, size=(5, 2)).astype(np.float32), [[0, 1], [0, 2], [3, 0], [4, 0], [1, 2]]),
    ]
