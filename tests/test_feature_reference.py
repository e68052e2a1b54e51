"""The numpy restatement of fi_points_describe / fi_feature_match (tests/feature_reference.py) held to answers known by hand,
so that the device, which tests/test_gpu_feature.py holds to the restatement bit for bit, is held to them too.  No GPU."""
import numpy as np

import feature_reference as FR


def flat_grid(side=9, z=2.0):
    x, y = np.meshgrid(np.arange(side, dtype=np.float32), np.arange(side, dtype=np.float32))
    P = np.stack([x.ravel(), y.ravel(), np.full(side * side, z, np.float32)], axis=1)
    return P, np.tile(np.float32([0, 0, 1]), (side * side, 1))


def bumpy_cloud(n=400, seed=2):
    """points with coordinates in 64ths over [0, 16) and unnormalised normals in 64ths: a quarter turn about z and an integer
    shift map them to other fp32 numbers exactly"""
    rng = np.random.default_rng(seed)
    P = (rng.integers(0, 16 * 64, (n, 3)) / 64.0).astype(np.float32)
    P[:, 2] = (np.round(64 * (2.0 + np.sin(P[:, 0] / 3.0) + np.cos(P[:, 1] / 2.0))) / 64.0).astype(np.float32)
    nrm = (rng.integers(-32, 33, (n, 3)) / 64.0).astype(np.float32)
    nrm[:, 2] = 1.0
    return P, nrm


def test_a_flat_grid_fills_one_bin_of_every_block():
    """every normal is +z and every neighbour lies in the plane, so for every pair: a_i = a_j = 0 (no swap, f_2 = 0, t_2 = 5.5,
    bin 5); v = e x n lies in the plane, f_1 = v . n = 0 (t_1 = 5.5, bin 5); x = n . n = 1, y = (n x v) . n = 0, so the
    pseudo-angle is 0 (t_3 = 2 * 2.75 = 5.5, bin 5).  S is 100 in bins 5, 16 and 27, and so is every neighbour's"""
    P, nrm = flat_grid()
    feat, valid, c, m = FR.describe(P, nrm, 9, parts=True)
    assert valid.all() and (m == 8).all()                                  # the point itself takes one of the nine places
    want = np.zeros(33, np.int64)
    want[[5, 16, 27]] = 8
    assert (c == want).all()
    inner = np.flatnonzero((P[:, 0] > 0) & (P[:, 0] < 8) & (P[:, 1] > 0) & (P[:, 1] < 8))
    for blk in range(3):
        block = feat[:, 11 * blk:11 * blk + 11]
        assert (block.sum(axis=1)[inner] == 100.0).all() and (block[inner, 5] == 100.0).all()
    assert (np.delete(feat, [5, 16, 27], axis=1) == 0).all()
    assert np.abs(feat[:, [5, 16, 27]] - 100.0).max() <= 100 * 2.0 ** -23     # (the border too, to fp32's rounding)


def test_a_quarter_turn_and_an_integer_shift_change_no_bit():
    """(x, y, z) -> (-y, x, z) + integers is exact on these coordinates, every sum of the contract over the first two axes
    commutes, and the cross products come out as each other's components: the descriptors are the same bytes"""
    P, nrm = bumpy_cloud()
    shift = np.float32([5, -3, 4])
    Q = np.stack([-P[:, 1], P[:, 0], P[:, 2]], axis=1) + shift
    assert np.array_equal((Q - shift).astype(np.float32), np.stack([-P[:, 1], P[:, 0], P[:, 2]], axis=1))
    qn = np.stack([-nrm[:, 1], nrm[:, 0], nrm[:, 2]], axis=1)
    for k in (8, 32):
        a, va = FR.describe(P, nrm, k)
        b, vb = FR.describe(Q, qn, k)
        assert va.all() and vb.all()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.allclose(a.reshape(-1, 3, 11).sum(axis=2), 100.0, atol=1e-3)
    assert len(np.unique(a, axis=0)) > 300                                 # (and they do tell points apart)


def test_points_without_a_descriptor():
    P, nrm = bumpy_cloud(60)
    P[3, 1] = np.nan
    nrm[7] = 0.0
    nrm[11, 0] = np.inf
    nrm[13, 2] = np.nan
    nrm[20] *= 7.5                                                         # a normal need not be a unit vector
    feat, valid, c, m = FR.describe(P, nrm, 8, parts=True)
    dead = [3, 7, 11, 13]
    assert not valid[dead].any() and (feat[dead] == 0).all() and (m[dead] == 0).all()
    assert valid[np.setdiff1d(np.arange(60), dead)].all()
    unit = nrm.copy()
    unit[20] /= 7.5
    assert np.allclose(FR.describe(P, unit, 8)[0], feat, atol=1e-3)
    # 40 copies of one point: the 32 places of the first 33 copies' lists hold copies only (w = 0), so they count no pair
    D = np.concatenate([np.repeat(P[:1], 40, axis=0), P[20:]])
    dn = np.concatenate([np.repeat(nrm[:1], 40, axis=0), nrm[20:]])
    feat, valid, c, m = FR.describe(D, dn, 32, parts=True)
    assert (m[:40] == 0).all() and not valid[:40].any() and (feat[:40] == 0).all() and valid[40:].all()
    assert (m[40:] <= 31).all()
    # alone; and two points whose normals lie along the line between them: e x n has no length, the pair is skipped
    feat, valid = FR.describe(P[:1], nrm[:1], 4)
    assert feat.shape == (1, 33) and not valid.any() and (feat == 0).all()
    two = np.float32([[0, 0, 0], [0, 0, 2]])
    feat, valid, c, m = FR.describe(two, np.float32([[0, 0, 1], [0, 0, -3]]), 4, parts=True)
    assert (m == 0).all() and not valid.any() and (feat == 0).all()
    # a finite max_distance that empties a list
    far = np.concatenate([P[20:], np.float32([[100, 100, 100]])])
    feat, valid = FR.describe(far, np.concatenate([nrm[20:], np.float32([[0, 0, 1]])]), 8, max_distance=5.0)
    assert valid[:-1].all() and not valid[-1]
    empty = FR.describe(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 8)
    assert empty[0].shape == (0, 33) and empty[1].shape == (0,)


def crowd(n=34):
    """n points 1e-30 apart on a line with +z normals: their fp32 squared distances are all 0, so every list of 32 is the points
    0 .. 31, and the points from 32 on are not in their own"""
    P = np.zeros((n, 3), np.float32)
    P[:, 0] = np.arange(n, dtype=np.float32) * np.float32(1e-30)
    return P, np.tile(np.float32([0, 0, 1]), (n, 1))


def test_a_list_without_the_point_itself_counts_thirty_two_pairs():
    """the fp64 distances of the crowd are not 0, so no pair is skipped: the points 0 .. 31 count 31 pairs and the others all
    32, and as on the flat grid every pair falls into bin 5 of its block"""
    P, nrm = crowd()
    feat, valid, c, m = FR.describe(P, nrm, 32, parts=True)
    assert valid.all() and m.tolist() == [31] * 32 + [32, 32]
    assert (c[:, [5, 16, 27]] == m[:, None]).all() and (np.delete(c, [5, 16, 27], axis=1) == 0).all()
    assert (np.delete(feat, [5, 16, 27], axis=1) == 0).all() and np.abs(feat[:, [5, 16, 27]] - 100.0).max() <= 100 * 2.0 ** -23
    # the same in the last bin of the second block: normals along the line, a_i = 1 for the points in front
    along = np.tile(np.float32([1, 0, 0]), (34, 1))
    feat, valid, c, m = FR.describe(P, along, 32, parts=True)
    assert (m == 0).all() and not valid.any()                              # (e x n has no length: nothing is counted)
    tilted = np.tile(np.float32([1, 0, 1]), (34, 1))
    feat, valid, c, m = FR.describe(P, tilted, 32, parts=True)
    assert m.tolist() == [31] * 32 + [32, 32] and c[33].max() == 32 and c[33].sum() == 96


def test_matching_ties_masks_and_mutual():
    b = np.float32([[0, 0], [2, 0], [2, 0], [5, 5], [np.nan, 0], [0, 2]])
    a = np.float32([[2, 0], [1, 1], [np.inf, 0], [5, 4], [0.5, 0.5]])
    idx, dist = FR.match(a, b)
    # row 1 is sqrt(2) from rows 0, 1, 2 and 5: the lowest wins; row 2 is not finite; b's row 4 is never a partner
    assert idx.tolist() == [1, 0, -1, 3, 0]
    assert dist.tolist() == [0.0, np.sqrt(np.float32(2)), np.inf, 1.0, np.sqrt(np.float32(0.5))]
    idx, dist = FR.match(a, b, valid_b=[0, 0, 1, 1, 1, 1])
    assert idx.tolist() == [2, 2, -1, 3, 2]                                # (row 4 is as far from b's row 2 as from its row 5)
    idx, dist = FR.match(a, b, valid_a=[1, 0, 1, 1, 1], valid_b=[0, 0, 0, 0, 1, 0])
    assert idx.tolist() == [-1] * 5 and np.isinf(dist).all()
    idx, _ = FR.match(a, np.zeros((0, 2), np.float32))
    assert idx.tolist() == [-1] * 5
    # mutual: b's rows 0 .. 5 go back to a's rows 4, 0, 0, 3, -, 1; only the matches that come back stay
    idx, dist = FR.match_mutual(a, b)
    assert idx.tolist() == [1, -1, -1, 3, 0] and np.isinf(dist[[1, 2]]).all() and dist[[0, 3]].tolist() == [0.0, 1.0]
    # the sum runs over ascending columns in fp32: 2^24 + 1 + 1 stays 2^24 one way and not the other
    big = np.float32([[4096.0, 1.0, 1.0]])
    assert FR.match(big, np.zeros((1, 3), np.float32))[1][0] == np.sqrt(np.float32(2 ** 24))
    assert FR.match(big[:, ::-1], np.zeros((1, 3), np.float32))[1][0] == np.sqrt(np.float32(2 ** 24 + 2))
