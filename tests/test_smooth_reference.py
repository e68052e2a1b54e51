"""The numpy restatement of the smoothing contract (tests/smooth_reference.py) held to facts that can be derived without it:
the closed-form shrinkage of a regular polygon, symmetry on a flat grid, a rim that stays in the lattice face it lies in, a
voxel staircase that gets smoother while Taubin's second step keeps its volume, the max_move bound, normals against the
extractor's, and the adjacency as a set.  No GPU."""
import math

import numpy as np
import pytest

import iso_reference as R
import mesh_parts_reference as M
import simplify_reference as S
import smooth_cases as K
import smooth_reference as T


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- the ranked sums are the serial sums ------------------------------------------------------------------------------

def _loop_smooth(v, idx, iterations, lam, mu, boundary, max_move):
    """fi_mesh_smooth's positions by a plain per-vertex loop over Python sets and floats (a Python float is an IEEE double)"""
    v = np.asarray(v, np.float32)
    nv, D = v.shape
    idx = np.asarray(idx, np.int64).reshape(-1, D)
    count = {}
    for row in idx:
        for a, b in ([(row[0], row[1]), (row[1], row[2]), (row[2], row[0])] if D == 3 else [(row[0], row[1])]):
            if a != b:
                key = (min(a, b), max(a, b))
                count[key] = count.get(key, 0) + 1
    N = [set() for _ in range(nv)]
    B = [set() for _ in range(nv)]
    degree = [0] * nv
    for (a, b), c in count.items():
        N[a].add(b), N[b].add(a)
        degree[a] += c
        degree[b] += c
        if c == 1:
            B[a].add(b), B[b].add(a)
    rim = [bool(B[i]) if D == 3 else degree[i] == 1 for i in range(nv)]
    sets = []
    for i in range(nv):
        if boundary == T.FREE or not rim[i]:
            sets.append(sorted(N[i]))
        elif boundary == T.SLIDE and D == 3:
            sets.append(sorted(B[i]))
        else:
            sets.append([])
    x0 = [[float(c) for c in p] for p in v]
    x = [list(p) for p in x0]
    lam, mu, m = float(np.float32(lam)), float(np.float32(mu)), float(np.float32(max_move))
    for _ in range(iterations):
        for f in ([lam, mu] if mu != 0 else [lam]):
            y = [list(p) for p in x]
            for i, s in enumerate(sets):
                for a in range(D):
                    if s:
                        acc = 0.0
                        for w in s:
                            acc = acc + x[w][a]
                        t = acc / float(len(s)) - x[i][a]
                        t = f * t
                        y[i][a] = x[i][a] + t
            x = y
        if m > 0:
            for i in range(nv):
                d = [x[i][a] - x0[i][a] for a in range(D)]
                s2 = d[0] * d[0] + d[1] * d[1]
                if D == 3:
                    s2 = s2 + d[2] * d[2]
                if s2 > m * m:
                    r = m / math.sqrt(s2)
                    x[i] = [x0[i][a] + d[a] * r for a in range(D)]
    return np.array(x, np.float64).reshape(nv, D).astype(np.float32)


def _loop_normals(v, idx):
    v = np.asarray(v, np.float32)
    nv, D = v.shape
    idx = np.asarray(idx, np.int64).reshape(-1, D)
    out = np.zeros((nv, D), np.float32)
    for i in range(nv):
        s = [0.0] * D
        for row in idx:
            if i not in row:
                continue
            q = [[float(c) for c in v[w]] for w in row]
            if D == 3:
                u = [q[1][d] - q[0][d] for d in range(3)]
                w = [q[2][d] - q[0][d] for d in range(3)]
                n = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
            else:
                n = [q[1][1] - q[0][1], -(q[1][0] - q[0][0])]
            s = [s[d] + n[d] for d in range(D)]
        l2 = s[0] * s[0] + s[1] * s[1]
        if D == 3:
            l2 = l2 + s[2] * s[2]
        ln = math.sqrt(l2)
        if ln > 0:
            out[i] = [np.float32(s[d] / ln) for d in range(D)]
    return out


@pytest.mark.parametrize("boundary", [T.FIXED, T.SLIDE, T.FREE])
def test_the_vectorised_sums_are_the_serial_ones(boundary):
    grid = K.flat_grid(5)
    bumpy = grid[0].copy()
    bumpy[:, 2] += np.random.default_rng(2).normal(scale=0.3, size=len(bumpy)).astype(np.float32)
    cases = [(name, v, t) for name, v, t in K.constructed()] + [("bumpy grid", bumpy, grid[1]), ("polygon",) + K.polygon(7)]
    for name, v, t in cases:
        v = np.asarray(v, np.float32)
        for mu, max_move in ((0.0, 0.0), (-0.53, 0.0), (-0.53, 0.05)):
            got, _n = T.smooth(v, None, t, 3, 0.5, mu, boundary, max_move)
            want = _loop_smooth(v, t, 3, 0.5, mu, boundary, max_move)
            assert np.array_equal(_bits(got), _bits(want)), (name, mu, max_move)
        assert np.array_equal(_bits(T.mesh_normals(v, t)), _bits(_loop_normals(v, t))), name


# ---- closed forms -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mu", [0.0, -0.53])
def test_regular_polygon_shrinks_by_the_closed_form(mu):
    n, radius, k, lam = 12, 5.0, 7, 0.5
    v, seg = K.polygon(n, radius, (7.0, 6.0))
    out, _ = T.smooth(v, None, seg, k, lam, mu, T.FREE)
    s = 1.0 - math.cos(2.0 * math.pi / n)
    want = radius * ((1.0 - lam * s) * (1.0 - float(np.float32(mu)) * s)) ** k
    r = np.sqrt(((out.astype(np.float64) - out.astype(np.float64).mean(axis=0)) ** 2).sum(axis=1))
    # four fp32 ulps at these coordinates: only the fp32 input and the final cast separate the two sides
    assert np.abs(r - want).max() <= 4e-6, np.abs(r - want).max()


def test_flat_grid():
    v, t, rim = K.flat_grid(6, 3.125)
    for mu in (0.0, -0.53):
        fixed, _ = T.smooth(v, None, t, 5, 0.5, mu, T.FIXED)
        # the rim is held, and an interior vertex's six neighbours lie symmetrically about it: nothing moves at all
        assert np.array_equal(_bits(fixed[rim]), _bits(v[rim])) and np.array_equal(_bits(fixed), _bits(v))
        free, _ = T.smooth(v, None, t, 5, 0.5, mu, T.FREE)
        assert np.array_equal(_bits(free[:, 2]), _bits(v[:, 2])) and not np.array_equal(free, v)


def test_a_rim_in_a_lattice_face_slides_in_it():
    pos, nrm, idx, _keys = K.cut_sphere()
    _v, _w, _eb, vb = T.adjacency(len(pos), idx, 3)
    assert (len(pos), int(vb.sum())) == (344, 40) and np.all(pos[vb, 0] == 19.0)
    slide, _ = T.smooth(pos, None, idx, 5, 0.5, -0.53, T.SLIDE)
    assert np.array_equal(_bits(slide[vb, 0]), _bits(pos[vb, 0]))              # x = 19 bit for bit ...
    assert np.all(np.abs(slide[vb, 1:] - pos[vb, 1:]).max(axis=1) > 0)         # ... and every rim vertex moved in the plane
    fixed, _ = T.smooth(pos, None, idx, 5, 0.5, -0.53, T.FIXED)
    assert np.array_equal(_bits(fixed[vb]), _bits(pos[vb])) and not np.array_equal(fixed[~vb], pos[~vb])


@pytest.fixture(scope="module")
def stairs():
    (pos, nrm, idx, keys), centre = K.staircase()
    assert (len(pos), len(idx)) == (1528, 3052)
    return pos, nrm, idx, keys, centre


@pytest.fixture(scope="module")
def faired(stairs):
    pos, nrm, idx, _keys, _c = stairs
    return {mu: T.smooth(pos, nrm, idx, 10, 0.5, mu)[0] for mu in (0.0, -0.53)}


def test_a_staircase_gets_smoother_and_taubin_keeps_its_volume(stairs, faired):
    pos, _nrm, idx, _keys, centre = stairs
    start = K.radial_rms_angle(pos, idx, centre)
    laplace, taubin = (K.radial_rms_angle(faired[mu], idx, centre) for mu in (0.0, -0.53))
    volume = [R.signed_measure(p, idx) for p in (pos, faired[0.0], faired[-0.53])]
    print("rms angle %.2f -> laplacian %.2f, taubin %.2f degrees; volume %.1f -> %.1f, %.1f" % (start, laplace, taubin, *volume))
    assert laplace < start and taubin < start
    assert abs(volume[2] - volume[0]) < abs(volume[1] - volume[0])


@pytest.mark.parametrize("max_move", [0.5, 0.25])
def test_max_move(stairs, faired, max_move):
    pos, nrm, idx, _keys, _c = stairs
    out, _ = T.smooth(pos, nrm, idx, 10, 0.5, 0.0, T.FIXED, max_move)
    moved = np.sqrt(((out.astype(np.float64) - pos.astype(np.float64)) ** 2).sum(axis=1))
    free = np.sqrt(((faired[0.0].astype(np.float64) - pos.astype(np.float64)) ** 2).sum(axis=1))
    # the cast is the only excess: half an ulp an axis, far below two ulps of the largest coordinate
    assert moved.max() <= max_move + 2.0 * float(np.spacing(np.abs(out).max()))
    assert (free > max_move).any() and moved.max() > 0.999 * max_move        # somebody was clamped


def test_invariance(stairs, faired):
    pos, nrm, idx, _keys, _c = stairs
    # the indices are untouched: watertight, oriented, a sphere
    assert R.watertight_oriented(idx) and R.euler_characteristic(len(pos), idx) == 2
    assert R.signed_measure(faired[-0.53], idx) > 0
    same, same_n = T.smooth(pos, nrm, idx, 0, 0.5, -0.53, T.FREE, 0.0, T.KEEP)
    assert np.array_equal(_bits(same), _bits(pos)) and np.array_equal(_bits(same_n), _bits(nrm))
    name, v, t = K.constructed()[5]
    v = v.copy()
    v[6] = [np.nan, np.inf, -np.inf]                                          # an unused vertex may be anything
    for boundary in (T.FIXED, T.SLIDE, T.FREE):
        out, _ = T.smooth(v, None, t, 4, 0.5, -0.53, boundary)
        assert np.array_equal(_bits(out[4:]), _bits(v[4:])), name            # unused: 4, 6, 7; isolated: 5 (only [5, 5, 5])
        assert (boundary == T.FIXED) == np.array_equal(out[:4], v[:4])       # (two triangles: every vertex is on the rim)
    v[1, 0] = np.inf
    with pytest.raises(T.Invalid):
        T.smooth(v, None, t, 1)
    with pytest.raises(T.Invalid):
        T.mesh_normals(v, t)


def test_options_out_of_range():
    v, t, _rim = K.flat_grid(3)
    for kw in ({"iterations": -1}, {"lam": -0.1}, {"lam": 1.5}, {"lam": np.nan}, {"mu": 0.1}, {"mu": -2.5}, {"mu": np.nan},
               {"max_move": -1.0}, {"max_move": np.nan}, {"boundary": 3}, {"boundary": -1}, {"normals_mode": 2}):
        with pytest.raises(T.Invalid):
            T.smooth(v, None, t, **kw)


# ---- normals ------------------------------------------------------------------------------------------------------------

def test_normals_agree_with_the_extractors():
    f, _c = S.sphere_field()
    pos, nrm, idx, _keys = R.extract(f, [24, 24, 24])
    dots = (T.mesh_normals(pos, idx).astype(np.float64) * nrm).sum(axis=1)
    print("3-D: least dot product %.4f" % dots.min())
    assert dots.min() >= 0.995
    pos, nrm, idx, _keys = R.extract(M.fixture_2d(), M.FIXTURE_2D_SIZES)
    dots = (T.mesh_normals(pos, idx).astype(np.float64) * nrm).sum(axis=1)
    print("2-D: least dot product %.4f" % dots.min())
    assert dots.min() >= 0.977


def test_normals_of_constructed_cases():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], np.float32)
    n = T.mesh_normals(v, [[0, 1, 2]])
    assert n[:3].tolist() == [[0, 0, 1]] * 3 and n[3].tolist() == [0, 0, 0]           # an unused vertex: zeros
    # a vertex named twice in one triangle counts once (such a triangle has no area: its normal is zero either way)
    w = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    once = T.mesh_normals(w, [[0, 1, 2], [0, 3, 1]])
    twice = T.mesh_normals(w, [[0, 1, 2], [0, 3, 1], [0, 0, 1]])
    assert np.array_equal(_bits(once), _bits(twice))
    name, fan, t = K.constructed()[4]
    assert not T.mesh_normals(fan, t).any(), name                                       # a zero-area fan: zeros
    seg = T.mesh_normals(np.array([[0, 0], [2, 0], [2, 3]], np.float32), [[0, 1], [1, 2]])
    assert seg[0].tolist() == [0, -1] and seg[2].tolist() == [1, 0]                     # the inside on the left
    assert np.allclose(seg[1], np.array([3, -2]) / math.sqrt(13))                       # length weights


def test_recompute_is_mesh_normals_of_keep(stairs):
    pos, nrm, idx, _keys, _c = stairs
    out, n = T.smooth(pos, nrm, idx, 3, 0.5, -0.53, T.FIXED, 0.0, T.RECOMPUTE)
    kept, kn = T.smooth(pos, nrm, idx, 3, 0.5, -0.53, T.FIXED, 0.0, T.KEEP)
    assert np.array_equal(_bits(out), _bits(kept)) and np.array_equal(_bits(kn), _bits(nrm))
    assert np.array_equal(_bits(n), _bits(T.mesh_normals(kept, idx)))
    assert T.smooth(pos, None, idx, 3)[1] is None


# ---- adjacency --------------------------------------------------------------------------------------------------------

def test_adjacency_is_a_set():
    cases = {name: (v, t) for name, v, t in K.constructed()}

    def rows_of(name, boundary=T.FREE):
        v, t = cases[name]
        off, nbr = T.rows(len(v), t, np.asarray(v).shape[1], boundary)
        return [nbr[off[i]:off[i + 1]].tolist() for i in range(len(v))]

    assert rows_of("duplicated triangles") == [[1, 2], [0, 2, 3, 4], [0, 1, 3], [1, 2, 4], [1, 3]]
    assert rows_of("a triangle and its reverse") == [[1, 2], [0, 2, 3], [0, 1, 3], [1, 2]]
    assert rows_of("repeated indices") == [[1, 2], [0, 2, 4], [0, 1, 4], [], [1, 2]]
    # an edge used three times is not a boundary edge: under SLIDE its ends average over their other (boundary) edges only
    v, t = cases["an edge used three times"]
    _v, _w, eb, vb = T.adjacency(5, t, 3)
    assert vb.all() and sorted(zip(_v[~eb].tolist(), _w[~eb].tolist())) == [(0, 1), (1, 0)]
    assert rows_of("an edge used three times", T.SLIDE) == [[2, 3, 4], [2, 3, 4], [0, 1], [0, 1], [0, 1]]
    assert rows_of("an edge used three times", T.FIXED) == [[]] * 5
    # duplicated triangles: every pair is used twice -- no boundary at all
    assert not T.adjacency(5, [[0, 1, 2], [0, 1, 2]], 3)[3].any()
    # 2-D: the ends of the chain are boundary; a doubled segment's end has degree 2 and is not
    assert rows_of("2-d: a chain, a doubled segment, a point", T.FIXED) == [[], [0, 2], [1, 3], [], [5], [4, 6], [], [], []]
    assert rows_of("2-d: a chain, a doubled segment, a point", T.SLIDE) == rows_of("2-d: a chain, a doubled segment, a point", T.FIXED)
    assert rows_of("2-d: a star", T.FREE) == [[1, 2, 3, 4], [0, 2], [0, 1], [0], [0]]
    assert rows_of("2-d: a star", T.FIXED) == [[1, 2, 3, 4], [0, 2], [0, 1], [], []]
