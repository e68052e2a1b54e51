"""The numpy restatement of the mesh sampling / deviation contract (tests/meshpts_reference.py) held to facts on the CPU: the
strata give every primitive its share, samples lie in their primitives and on the surface, simplification with quadric
placement keeps a cube and mean placement does not, shifted copies are as far away as they were shifted, degenerate and
unused geometry is never sampled, and the fixed-order sums and the stratum search agree with plain loops."""
import functools
import math

import numpy as np
import pytest

import meshpts_reference as P
import simplify_reference as S
import smooth_cases as K


@functools.lru_cache(maxsize=None)
def cube():
    v, t = S.cube_mesh()
    assert v.shape == (866, 3) and t.shape == (1728, 3) and v.max() == 11.25
    return v, t


@functools.lru_cache(maxsize=None)
def coarse_cube(placement):
    v, t = cube()
    r = S.simplify(v, None, t, 3.0, None, placement)
    assert r.vertices.shape == (56, 3) and r.indices.shape == (108, 3)
    return r.vertices, r.indices


# ---- the cube: counts and placement -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_cube_sample_counts_and_placement(n):
    v, t = cube()
    pos, nrm, prim = P.sample(v, None, t, n, 7)
    q, _C, T = P.integer_weights(v, t)
    worst = np.abs(np.bincount(prim, minlength=len(t)) - n * q.astype(np.float64) / T).max()
    print("n = %d: the worst |count - n q / T| = %.3f" % (n, worst))
    assert worst < 2.0
    assert np.all(np.diff(prim) >= 0)
    tri = v[t[prim]]
    assert np.all(pos >= tri.min(axis=1)) and np.all(pos <= tri.max(axis=1))
    assert np.abs(np.sqrt((nrm.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() < 1e-6
    assert pos.dtype == np.float32 and nrm.dtype == np.float32 and prim.dtype == np.int64


def test_cube_samples_lie_on_the_cube():
    v, t = cube()
    of_s, of_v, vd = P.deviation(v, t, v, t, 5000, 7)
    ulp = float(np.spacing(np.float32(11.25)))
    print("self-distance of 5000 samples: max %.3g (one ulp at 11.25: %.3g)" % (of_s["max"], ulp))
    assert of_s["queries"] == of_s["counted"] == 5000 and of_s["max"] <= 4 * ulp
    assert of_v["queries"] == of_v["counted"] == len(v) and of_v["max"] == 0.0 and not vd.any()


def test_cube_simplified():
    v, t = cube()
    for placement, name in ((S.QUADRIC, "quadric"), (S.MEAN, "mean")):
        cv, ct = coarse_cube(placement)
        for what, (a, b) in (("simplified -> original", ((cv, ct), (v, t))), ("original -> simplified", ((v, t), (cv, ct)))):
            of_s, of_v, _vd = P.deviation(a[0], a[1], b[0], b[1], 4096, 0)
            print("%s, %s: max %.3g mean %.3g rms %.3g (vertices: max %.3g)" % (name, what, of_s["max"], of_s["mean"], of_s["rms"], of_v["max"]))
            assert of_s["counted"] == 4096
            if placement == S.QUADRIC:
                assert of_s["max"] < 1e-5
            else:
                assert of_s["max"] > 0.5
            assert 0.0 <= of_s["mean"] <= of_s["rms"] <= of_s["max"]


# ---- shifted copies ---------------------------------------------------------------------------------------------------

def test_shifted_flat_grid():
    v, t, _rim = K.flat_grid(6, 3.125)
    h = 0.375
    w = v + np.array([0, 0, h], np.float32)
    for a, b in ((v, w), (w, v)):
        of_s, of_v, vd = P.deviation(a, t, b, t, 1000, 3)
        for r, n in ((of_s, 1000), (of_v, len(v))):
            assert r["queries"] == r["counted"] == n and r["beyond"] == 0 and r["invalid"] == 0
            assert r["max"] == h and r["mean"] == h and r["rms"] == h and r["at"] == 0
        assert np.all(vd == np.float32(h))
        assert np.array_equal(of_v["where"], a[0])


def test_shifted_square():
    v, seg = S.square_polyline()
    w = v + np.array([0.25, 0.0], np.float32)
    of_s, of_v, vd = P.deviation(v, seg, w, seg, 500, 1)
    lo, hi = 1.5, 5.5
    on_parallel_side = ((v[:, 1] == lo) | (v[:, 1] == hi)) & (v[:, 0] >= lo + 0.25)   # (the left corners face the shifted corners)
    assert np.array_equal(vd, np.where(on_parallel_side, 0.0, 0.25).astype(np.float32))
    assert of_v["max"] == 0.25 and of_v["at"] == int(np.flatnonzero(~on_parallel_side)[0])
    assert of_s["counted"] == 500 and of_s["max"] <= 0.25 and 0.0 < of_s["mean"] < 0.25
    pos, nrm, prim = P.sample(v, None, seg, 64, 5)
    # counter-clockwise with the inside on the left: the normals point away from the centre
    assert np.all(((pos - np.float32(3.5)) * nrm).sum(axis=1) > 0)


# ---- constructed cases ------------------------------------------------------------------------------------------------

def test_constructed_cases():
    for name, v, t in K.constructed():
        v = np.asarray(v, np.float32)
        D = v.shape[1]
        t = np.asarray(t, np.int32).reshape(-1, D)
        q, _C, T = P.integer_weights(v, t)
        used = np.zeros(len(v), bool)
        used[t.reshape(-1)] = True
        if T == 0:
            with pytest.raises(P.Invalid):
                P.sample(v, None, t, 10, 0)
            of_s, of_v, vd = P.deviation(v, t, v, t, 10, 0)
            assert of_s == {**P.nothing(), "where": of_s["where"]} and not of_s["where"].any() and of_s["at"] == -1, name
        else:
            pos, _n, prim = P.sample(v, None, t, 300, 2)
            assert np.all(q[prim] > 0), name
            rows = t[prim]
            assert np.all(rows[:, 0] != rows[:, 1]), name                      # a repeated index spans no measure
            if D == 3:
                assert np.all((rows[:, 1] != rows[:, 2]) & (rows[:, 0] != rows[:, 2])), name
            of_s, of_v, vd = P.deviation(v, t, v, t, 300, 2)
            assert of_s["queries"] == 300, name
        assert of_v["queries"] == used.sum(), name
        assert np.array_equal(np.isnan(vd), ~used), name
        for r in (of_s, of_v):
            assert r["counted"] + r["beyond"] + r["invalid"] == r["queries"], name
    assert P.integer_weights(*[np.asarray(x) for x in K.constructed()[4][1:]])[2] == 0   # the zero-area fan


def test_non_finite_vertices_and_max_distance():
    v, t = cube()
    w = v.copy()
    w[t[5, 1], 2] = np.nan
    of_s, of_v, vd = P.deviation(w, t, v, t, 500, 0)
    assert of_v["invalid"] == 1 and of_v["counted"] == len(v) - 1 and np.isnan(vd).sum() == 1
    assert of_s["counted"] == 500 and of_s["invalid"] == 0                     # (its triangles weigh nothing: never sampled)
    cv, ct = coarse_cube(S.MEAN)
    of_s, of_v, _vd = P.deviation(v, t, cv, ct, 500, 0, max_distance=0.25)
    for r in (of_s, of_v):
        assert r["beyond"] > 0 and r["counted"] > 0 and r["counted"] + r["beyond"] + r["invalid"] == r["queries"]
        assert r["max"] <= 0.25
    for bad in (np.nan, -1.0):
        with pytest.raises(P.Invalid):
            P.deviation(v, t, v, t, 10, 0, bad)
    with pytest.raises(P.Invalid):
        P.deviation(v, t, *S.square_polyline(), 10)                            # a 3-D mesh against a 2-D surface
    with pytest.raises(P.Invalid):
        P.sample(v, None, t, -1)
    with pytest.raises(P.Invalid):
        P.sample(v, None, t, 5, 0, P.VERTEX, True)
    with pytest.raises(P.Unsupported):
        P.sample(v, None, t, 2 ** 31)
    assert P.sample(v, None, t, 0)[0].shape == (0, 3)


def test_vertex_normals_mode():
    v, t = cube()
    centre = np.float32(6.75)
    nv = (v - centre) / np.linalg.norm(v - centre, axis=1, keepdims=True)
    pos, nrm, prim = P.sample(v, nv.astype(np.float32), t, 400, 9, P.VERTEX)
    assert np.abs(np.sqrt((nrm.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() < 1e-6
    face = P.sample(v, None, t, 400, 9, P.FACE)[1]
    assert (nrm * face).sum(axis=1).min() > 0.5
    # zero vertex normals fall back to the face normal
    again = P.sample(v, np.zeros_like(v), t, 400, 9, P.VERTEX)[1]
    assert np.array_equal(again.view(np.uint32), face.view(np.uint32))
    other = P.sample(v, None, t, 400, 10)[0]
    assert not np.array_equal(other, pos)


# ---- summation and search ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 70000])
def test_tree_sum(n):
    x = np.random.default_rng(n).uniform(0.0, 3.0, size=n) ** 3
    want = math.fsum(x)
    assert abs(float(P.tree_sum(x)) - want) <= 1e-12 * want
    # the tree, written out for the first block
    s = np.zeros(256)
    s[:min(n, 256)] = x[:256]
    w = 128
    while w:
        for k in range(w):
            s[k] = s[k] + s[k + w]
        w //= 2
    assert float(P.tree_sum(x[:256])) == s[0]


def test_stratum_search_against_a_loop():
    v, t = cube()
    _q, C, T = P.integer_weights(v, t)
    n, seed = 777, 12345678901234567890
    prim = P.sample(v, None, t, n, seed)[2]
    mask = (1 << 64) - 1
    for i in range(n):
        z = (seed + (3 * i + 1) * 0x9E3779B97F4A7C15) & mask
        z ^= z >> 30
        z = (z * 0xBF58476D1CE4E5B9) & mask
        z ^= z >> 27
        z = (z * 0x94D049BB133111EB) & mask
        z ^= z >> 31
        xi = (z >> 11) * 2.0 ** -53
        y = ((float(i) + xi) / float(n)) * float(T)
        tt = min(int(y), T - 1)
        p = 0
        while int(C[p]) <= tt:
            p += 1
        assert p == prim[i], i
