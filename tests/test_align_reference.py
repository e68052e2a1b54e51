"""The numpy restatement of fi_align_correspondences (tests/align_reference.py) held to answers known by hand, and the planted
case of DESIGN.md 4.22 -- two scans of one bumpy surface, 97 degrees and metres apart -- on the restatements alone
(feature_reference, align_reference, register_reference), so that the device, which tests/test_gpu_align.py holds to the
restatements bit for bit, is held to them too.  No GPU."""
import numpy as np
import pytest

import align_reference as AR
import feature_reference as FR
import register_reference as RR

QUARTER = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])     # 90 degrees about z: (x, y, z) -> (-y, x, z)
SHIFT = np.array([5.0, -3.0, 4.0])


def moved_exactly(P):
    """P (integers in fp32) turned by QUARTER and shifted by SHIFT: exact in fp32"""
    return (np.asarray(P, np.float64) @ QUARTER.T + SHIFT).astype(np.float32)


def lattice_pairs(side=4):
    g = np.stack(np.meshgrid(*[np.arange(side, dtype=np.float32)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return g, moved_exactly(g)


def _truth():
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = QUARTER, SHIFT
    return T


def test_three_exact_pairs_give_the_motion():
    """a right triangle with legs 3 and 6: whichever order a hypothesis draws its corners in, its frame vectors are the
    triangle's edges over their lengths and cross products of those -- a dozen roundings of numbers of magnitude <= 10, far
    inside 1e-13"""
    src = np.float32([[0, 0, 0], [3, 0, 0], [0, 6, 0]])
    tgt = moved_exactly(src)
    out, inl = AR.align(src, tgt, [0, 1, 2], [0, 1, 2], 1e-6, similarity=0.9, max_trials=64, confidence=0.0)
    assert out["found"] == 1 and out["pairs"] == 3 and out["live"] == 3 and out["trials"] == 64 and out["inliers"] == 3
    assert 0 < out["valid"] < 64                      # a draw repeats a pair about seven times in nine
    assert np.abs(out["transform"] - _truth()).max() <= 1e-13 and out["rms"] <= 1e-13
    assert out["transform"][3].tolist() == [0.0, 0.0, 0.0, 1.0] and inl.tolist() == [1, 1, 1]
    # the corners drawn in the order 0, 1, 2 divide by 3 and 6 only, and both centroids are integers: that hypothesis is exact
    R, t, valid = AR.hypotheses(src.astype(np.float64), tgt.astype(np.float64), 0, np.arange(4096))
    c = np.arange(4096, dtype=np.uint64)
    j = [np.minimum(np.floor(AR.uniform(0, 3 * c + np.uint64(k)) * 3.0).astype(int), 2) for k in range(3)]
    at = np.flatnonzero((j[0] == 0) & (j[1] == 1) & (j[2] == 2))
    assert len(at) and valid[at].all()
    assert np.array_equal(R[at[0]], QUARTER) and t[at[0]].tolist() == SHIFT.tolist()


def test_fewer_than_three_live_pairs():
    src, tgt = lattice_pairs(2)
    out, inl = AR.align(src, tgt, [0, 1], [0, 1], 0.1)
    assert (out["found"], out["pairs"], out["live"], out["trials"], out["valid"]) == (0, 2, 2, 0, 0) and not inl.any()
    assert np.array_equal(out["transform"], np.eye(4)) and out["rms"] == 0.0
    bad = src.copy()
    bad[2, 1] = np.nan
    bad_t = tgt.copy()
    bad_t[3, 0] = np.inf
    # pairs 2 and 3 are not finite, 4 .. 7 are out of range: two live pairs are left
    out, inl = AR.align(bad, bad_t, [0, 1, 2, 3, -1, 8, 4, 5], [0, 1, 2, 3, 4, 5, -1, 8], 0.1)
    assert (out["found"], out["pairs"], out["live"], out["trials"]) == (0, 8, 2, 0) and inl.shape == (8,) and not inl.any()
    out, inl = AR.align(src, tgt, [], [], 0.1)
    assert (out["found"], out["pairs"], out["live"]) == (0, 0, 0) and inl.shape == (0,)


def test_collinear_triples_form_no_frame():
    src = np.stack([np.arange(12.0), 2.0 * np.arange(12.0), -np.arange(12.0)], axis=1).astype(np.float32)
    tgt = moved_exactly(src)
    idx = np.arange(12)
    out, inl = AR.align(src, tgt, idx, idx, 0.1, similarity=0.0, max_trials=500, confidence=0.0)
    assert (out["found"], out["live"], out["trials"], out["valid"], out["inliers"]) == (0, 12, 500, 0, 0) and not inl.any()
    assert np.array_equal(out["transform"], np.eye(4))
    # a source of one point repeated: the first edge has no length
    out, _ = AR.align(np.repeat(src[:1], 12, axis=0), tgt, idx, idx, 0.1, similarity=0.0, max_trials=100)
    assert out["found"] == 0 and out["valid"] == 0 and out["trials"] == 100


def test_the_edge_test_at_its_boundary():
    """the target is the source at half its size, in powers of two: every target edge is exactly half its source edge, so
    min = 0.25 max exactly; similarity 0.5 squares to 0.25 and accepts, the next float above 0.5 refuses"""
    src = np.float32([[0, 0, 0], [4, 0, 0], [0, 8, 0], [0, 0, 16], [4, 8, 16]])
    tgt = (0.5 * src).astype(np.float32)
    idx = np.arange(5)
    at = AR.align(src, tgt, idx, idx, 0.1, similarity=0.5, max_trials=200, confidence=0.0)[0]
    above = AR.align(src, tgt, idx, idx, 0.1, similarity=np.nextafter(np.float32(0.5), np.float32(1.0)), max_trials=200, confidence=0.0)[0]
    free = AR.align(src, tgt, idx, idx, 0.1, similarity=0.0, max_trials=200, confidence=0.0)[0]
    assert at["found"] == 1 and at["valid"] == free["valid"] > 0
    assert above["found"] == 0 and above["valid"] == 0 and above["trials"] == 200
    # an exact copy passes at similarity 1
    one = AR.align(src, src.copy(), idx, idx, 0.1, similarity=1.0, max_trials=200, confidence=0.0)[0]
    assert one["found"] == 1 and one["valid"] == free["valid"] and one["inliers"] == 5


def test_equal_counts_go_to_the_lowest_hypothesis():
    src, tgt = lattice_pairs()
    idx = np.arange(len(src))
    out, inl = AR.align(src, tgt, idx, idx, 1e-6, similarity=0.9, max_trials=3000, confidence=0.0, seed=5)
    assert out["inliers"] == 64 and inl.all()
    X, Y = src.astype(np.float64), tgt.astype(np.float64)
    R, t, valid = AR.hypotheses(X, Y, 5, np.arange(3000), 0.9)
    sc = AR.scores(X, Y, R, t, valid, 1e-6)
    full = np.flatnonzero(sc == 64)
    assert len(full) > 10 and out["valid"] == int(valid.sum())             # many hypotheses tie at the top
    first = full[0]
    assert out["transform"][:3, :3].tobytes() == R[first].tobytes() and out["transform"][:3, 3].tobytes() == t[first].tobytes()
    assert any(R[h].tobytes() != R[first].tobytes() for h in full[1:])     # (and they are not all the same bytes)


def test_the_stop_rule():
    # q^T by the contract's multiplications against the power itself
    for b, live, T in ((13, 200, 16384), (13, 200, 32768), (50, 1000, 16384), (999, 1000, 3)):
        r = (1.0 - (b / live) ** 3) ** T
        if abs(r - 1e-3) > 1e-4:                                           # (away from the edge both must agree)
            assert AR.confident(b, live, T, 0.999) == (r <= 1e-3), (b, live, T)
    assert AR.confident(200, 200, 1, 0.999999) and not AR.confident(1, 200, 16384, 0.5)
    # one batch: every pair fits, so the first batch's best has w = 1
    src, tgt = lattice_pairs()
    idx = np.arange(64)
    out, _ = AR.align(src, tgt, idx, idx, 1e-6, similarity=0.9, max_trials=50000, confidence=0.999)
    assert out["trials"] == AR.BATCH and out["inliers"] == 64
    # several batches: 13 of 200 pairs fit, w^3 = 2.7e-4, and (1 - w^3)^T falls below 1e-3 between 16384 and 32768
    src, tgt, _, _ = AR.moved_pairs(3, 200, 0.0, noise=0.0)
    tgt[:13] = moved_exactly(np.round(src[:13]))
    src[:13] = np.round(src[:13])
    out, inl = AR.align(src, tgt, np.arange(200), np.arange(200), 1e-3, similarity=0.0, max_trials=100000, confidence=0.999, seed=1)
    assert out["inliers"] == 13 and inl[:13].all() and not inl[13:].any()
    assert out["trials"] == 2 * AR.BATCH
    # all of them: confidence 0 never stops, and the last batch is partial
    out, _ = AR.align(src, tgt, np.arange(200), np.arange(200), 1e-3, similarity=0.0, max_trials=40000, confidence=0.0, seed=1)
    assert out["trials"] == 40000 and out["inliers"] == 13 and out["valid"] <= 40000


# ---- the planted case ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    sp, sn, tp, tn, R0, shift = AR.planted_scans()
    fs, vs = FR.describe(sp, sn, 32)
    ft, vt = FR.describe(tp, tn, 32)
    matches, _ = FR.match(fs, ft, vs, vt)
    out, inl = AR.align(sp, tp, np.arange(len(sp)), matches, 1.0, similarity=0.9, max_trials=16384, confidence=0.0)
    return dict(sp=sp, sn=sn, tp=tp, tn=tn, R0=R0, shift=shift, matches=matches, out=out, inl=inl, vs=vs, vt=vt)


def test_planted_scans_come_within_ten_degrees(planted):
    p = planted
    out = p["out"]
    where = p["sp"].astype(np.float64) @ p["R0"].T + p["shift"]                 # the source points in the target's frame
    right = np.linalg.norm(p["tp"][np.maximum(p["matches"], 0)] - where, axis=1) < 1.5
    right &= p["matches"] >= 0
    angle = AR.angle_between(out["transform"][:3, :3], p["R0"])
    print("planted: source %d target %d matched %d right %.3f valid %d inliers %d angle %.3f rms %.4f"
          % (len(p["sp"]), len(p["tp"]), int((p["matches"] >= 0).sum()), right.mean(), out["valid"], out["inliers"], angle, out["rms"]))
    assert out["found"] == 1 and out["trials"] == 16384
    assert angle < 10.0
    assert p["inl"][right].sum() > p["inl"][~right].sum()                     # the motion keeps the right matches


def test_planted_scans_refine_to_the_true_pose(planted):
    p = planted
    target = RR.Target(points=p["tp"], normals=p["tn"])
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = p["R0"], p["shift"]
    run = lambda initial: RR.register(target, p["sp"], max_distance=3.0, initial=initial)  # noqa: E731
    got, true, idle = run(p["out"]["transform"]), run(T0), run(None)
    print("planted: rms from the alignment %.6f (%d steps, %d counted), from the true pose %.6f, from the identity %.6f (%d counted)"
          % (got["rms"], got["iterations"], got["counted"], true["rms"], idle["rms"], idle["counted"]))
    assert got["rms"] <= 1.01 * true["rms"]
    assert AR.angle_between(got["transform"][:3, :3], p["R0"]) < 1.0
    assert idle["counted"] == 0 or idle["rms"] > 5.0 * true["rms"]
