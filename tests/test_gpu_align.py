"""Coarse alignment on the device (fi_align.hip through align_correspondences, register_global and the raw
fi_align_correspondences) against the numpy restatement of the contract (tests/align_reference.py): the inlier mask
array-equal, every integer of the result equal and every double as a bit pattern.  The pair counts where a tile of the score,
a chunk of the tree sum and a wave end, trial counts on both sides of a batch, the edge test on and off, inlier shares of a
tenth and all, pairs that are out of range or not finite, the cases of tests/test_align_reference.py with answers known by
hand, the stop rule after one batch and at the end, the planted scans end to end, repeated calls, the error codes, and device
tensors through a child process."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import align_reference as AR
import feature_reference as FR
import register_reference as RR
from test_align_reference import lattice_pairs, moved_exactly

pytestmark = pytest.mark.gpu

COUNTS = [0, 2, 3, 255, 256, 257, 1000]                  # both sides of a tile and a chunk (256); four of them
MANY = [16384, 16385]                                    # all inliers: 64 chunks, one load of the ordered sum, and a 65th
TRIALS = [1, 16383, 16384, 16385, 40000]                # both sides of a batch (16384), two batches and a partial one
INTS = ("found", "pairs", "live", "trials", "valid", "inliers")


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist()


def _same(got, want, what=""):
    for key in INTS:
        assert int(got[key]) == int(want[key]), (what, key, got, want)
    assert got["transform"].dtype == np.float64 and got["transform"].shape == (4, 4), what
    assert _bits(got["transform"]) == _bits(want["transform"]), (what, got, want)
    assert _bits(got["rms"]) == _bits(want["rms"]), (what, got, want)


def _raw(src, tgt, si, ti, threshold=0.1, similarity=0.9, max_trials=1000, confidence=0.999, seed=0, memory=0, **over):
    """the C entry with host buffers -> (code, result dict, inliers)"""
    from field_interpolation_amd import _capi
    from field_interpolation_amd.api import _alignment_dict
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    si, ti = np.ascontiguousarray(si, np.int64), np.ascontiguousarray(ti, np.int64)
    opt = _capi.FiAlignOptions(threshold, similarity, max_trials, confidence, seed)
    res, inl = _capi.FiAlignment(), np.full(len(si), 7, np.uint8)
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None  # noqa: E731
    args = dict(ns=len(src), ps=ptr(src), nt=len(tgt), pt=ptr(tgt), m=len(si), psi=ptr(si), pti=ptr(ti), opt=C.byref(opt), out=C.byref(res),
                inl=ptr(inl))
    args.update(over)
    code = _capi.lib().fi_align_correspondences(args["ns"], args["ps"], args["nt"], args["pt"], args["m"], args["psi"], args["pti"], args["opt"],
                                                args["out"], args["inl"], memory)
    return code, _alignment_dict(res), inl


def _check(fi, src, tgt, si, ti, what="", **kw):
    """align_correspondences and the raw entry against the restatement"""
    want, want_inl = AR.align(src, tgt, si, ti, **kw)
    got, inl = fi.align_correspondences(src, tgt, np.asarray(si, np.int64), np.asarray(ti, np.int64), **kw)
    assert inl.dtype == np.bool_ and np.array_equal(inl, want_inl.astype(bool)), (what, np.flatnonzero(inl != want_inl.astype(bool))[:5])
    _same(got, want, what)
    code, got, inl = _raw(src, tgt, si, ti, **kw)
    assert code == 0 and np.array_equal(inl, want_inl), what
    _same(got, want, what)
    return want, want_inl


@pytest.mark.parametrize("share", [0.1, 1.0])
@pytest.mark.parametrize("similarity", [0.0, 0.9])
def test_sizes(fi, similarity, share):
    for m in COUNTS + (MANY if share == 1.0 else []):
        src, tgt, _, _ = AR.moved_pairs(10 + m, m, share)
        idx = np.arange(m)
        want, _ = _check(fi, src, tgt, idx, idx, (m, similarity, share), threshold=0.05, similarity=similarity, max_trials=3000,
                         confidence=0.0, seed=m)
        assert want["trials"] == (3000 if m >= 3 else 0)
        if m >= 255 and share == 1.0:
            assert want["found"] == 1 and want["inliers"] > 0.5 * m
        if m in MANY:
            assert want["inliers"] == m


@pytest.mark.parametrize("confidence", [0.0, 0.999])
@pytest.mark.parametrize("similarity", [0.0, 0.9])
def test_trial_counts(fi, similarity, confidence):
    src, tgt, _, _ = AR.moved_pairs(7, 257, 0.5)
    idx = np.arange(257)
    for trials in TRIALS:
        want, _ = _check(fi, src, tgt, idx, idx, (similarity, confidence, trials), threshold=0.05, similarity=similarity, max_trials=trials,
                         confidence=confidence, seed=3)
        assert want["trials"] == (trials if confidence == 0.0 else min(trials, AR.BATCH))      # w = 0.5 stops after a batch


def test_pairs_out_of_range_and_not_finite(fi):
    src, tgt, _, _ = AR.moved_pairs(21, 600, 0.6)
    rng = np.random.default_rng(4)
    si, ti = rng.permutation(600), np.arange(600)
    tgt = tgt[si]                                                          # pair c is (src[si[c]], tgt[c]): the partners still
    tgt, src = tgt.copy(), src.copy()
    si = si.astype(np.int64)
    ti = ti.astype(np.int64)
    si[::17], ti[5::23] = -1, 600
    si[3::41], ti[7::31] = 2 ** 40, -2 ** 40
    src[::13, 1], tgt[4::19, 0], tgt[9::29, 2] = np.nan, np.inf, -np.inf
    want, inl = _check(fi, src, tgt, si, ti, "holes", threshold=0.05, max_trials=5000, seed=2)
    ok = (si >= 0) & (si < 600) & (ti >= 0) & (ti < 600)
    ok[ok] = np.isfinite(src[si[ok]]).all(axis=1) & np.isfinite(tgt[ti[ok]]).all(axis=1)
    assert want["live"] == int(ok.sum()) < 500 and not inl[~ok].any() and want["found"] == 1
    # repeated pairs and fewer source points than pairs
    si = rng.integers(0, 50, 400)
    _check(fi, src[:50], tgt, si, rng.integers(0, 600, 400), "repeats", threshold=0.5, similarity=0.0, max_trials=2000, seed=9)


def test_answers_known_by_hand(fi):
    src = np.float32([[0, 0, 0], [3, 0, 0], [0, 6, 0]])
    want, _ = _check(fi, src, moved_exactly(src), [0, 1, 2], [0, 1, 2], "three pairs", threshold=1e-6, max_trials=64, confidence=0.0)
    assert want["inliers"] == 3
    src, tgt = lattice_pairs(2)
    want, _ = _check(fi, src, tgt, [0, 1], [0, 1], "two pairs", threshold=0.1)
    assert (want["found"], want["live"], want["trials"]) == (0, 2, 0)
    line = np.stack([np.arange(12.0), 2.0 * np.arange(12.0), -np.arange(12.0)], axis=1).astype(np.float32)
    idx = np.arange(12)
    want, _ = _check(fi, line, moved_exactly(line), idx, idx, "collinear", threshold=0.1, similarity=0.0, max_trials=500, confidence=0.0)
    assert (want["found"], want["valid"], want["trials"]) == (0, 0, 500)
    half = np.float32([[0, 0, 0], [4, 0, 0], [0, 8, 0], [0, 0, 16], [4, 8, 16]])
    idx = np.arange(5)
    at, _ = _check(fi, half, 0.5 * half, idx, idx, "edge test at", threshold=0.1, similarity=0.5, max_trials=200, confidence=0.0)
    above, _ = _check(fi, half, 0.5 * half, idx, idx, "edge test above", threshold=0.1, similarity=float(np.nextafter(np.float32(0.5), np.float32(1))),
                      max_trials=200, confidence=0.0)
    assert at["found"] == 1 and above["found"] == 0 and above["valid"] == 0
    src, tgt = lattice_pairs()
    idx = np.arange(64)
    want, inl = _check(fi, src, tgt, idx, idx, "ties", threshold=1e-6, max_trials=3000, confidence=0.0, seed=5)
    assert want["inliers"] == 64 and inl.all()
    got, inl = fi.align_correspondences(src, tgt, np.zeros(0, np.int64), np.zeros(0, np.int64), 0.1)
    assert not got["found"] and inl.shape == (0,) and np.array_equal(got["transform"], np.eye(4))
    # a threshold of +inf takes every live pair; of 0 only exact ones
    _check(fi, src, tgt, idx, idx, "threshold inf", threshold=math.inf, max_trials=100)
    _check(fi, src, tgt, idx, idx, "threshold 0", threshold=0.0, max_trials=3000, confidence=0.0)


def test_the_stop_rule(fi):
    src, tgt = lattice_pairs()
    idx = np.arange(64)
    want, _ = _check(fi, src, tgt, idx, idx, "one batch", threshold=1e-6, max_trials=50000)
    assert want["trials"] == AR.BATCH
    src, tgt, _, _ = AR.moved_pairs(3, 200, 0.0, noise=0.0)
    tgt[:13] = moved_exactly(np.round(src[:13]))
    src[:13] = np.round(src[:13])
    idx = np.arange(200)
    want, _ = _check(fi, src, tgt, idx, idx, "two batches", threshold=1e-3, similarity=0.0, max_trials=100000, seed=1)
    assert want["trials"] == 2 * AR.BATCH and want["inliers"] == 13
    want, _ = _check(fi, src, tgt, idx, idx, "to the end", threshold=1e-3, similarity=0.0, max_trials=40000, confidence=0.0, seed=1)
    assert want["trials"] == 40000


@pytest.fixture(scope="module")
def planted():
    sp, sn, tp, tn, R0, shift = AR.planted_scans()
    fs, vs = FR.describe(sp, sn, 32)
    ft, vt = FR.describe(tp, tn, 32)
    matches, _ = FR.match(fs, ft, vs, vt)
    mutual, _ = FR.match_mutual(fs, ft, vs, vt)
    return dict(sp=sp, sn=sn, tp=tp, tn=tn, R0=R0, matches=matches, mutual=mutual)


def test_planted_scans_end_to_end(fi, planted):
    p = planted
    kw = dict(similarity=0.9, max_trials=16384, confidence=0.0)
    want, want_inl = AR.align(p["sp"], p["tp"], np.arange(len(p["sp"])), p["matches"], 1.0, **kw)
    alignment, registration = fi.register_global(p["sp"], p["sn"], p["tp"], p["tn"], 1.0, refine=False, **kw)
    assert registration is None
    assert np.array_equal(alignment["matches"], p["matches"]) and np.array_equal(alignment["mask"], want_inl.astype(bool))
    _same(alignment, want, "planted")
    assert AR.angle_between(alignment["transform"][:3, :3], p["R0"]) < 10.0
    alignment, registration = fi.register_global(p["sp"], p["sn"], p["tp"], p["tn"], 1.0, **kw)
    _same(alignment, want, "planted, refined")
    ref = RR.register(RR.Target(points=p["tp"], normals=p["tn"]), p["sp"], max_distance=3.0, initial=want["transform"])
    assert _bits(registration["transform"]) == _bits(ref["transform"]) and _bits(registration["rms"]) == _bits(ref["rms"])
    assert registration["iterations"] == ref["iterations"] and registration["counted"] == ref["counted"] == len(p["sp"])
    assert AR.angle_between(registration["transform"][:3, :3], p["R0"]) < 1.0
    # mutual matches: fewer pairs, the same contract
    want, want_inl = AR.align(p["sp"], p["tp"], np.arange(len(p["sp"])), p["mutual"], 1.0, **kw)
    alignment, _ = fi.register_global(p["sp"], p["sn"], p["tp"], p["tn"], 1.0, mutual=True, refine=False, **kw)
    assert np.array_equal(alignment["matches"], p["mutual"]) and want["live"] == int((p["mutual"] >= 0).sum()) < len(p["sp"])
    _same(alignment, want, "planted, mutual")


def test_repeated_calls_return_the_same_bytes(fi):
    src, tgt, _, _ = AR.moved_pairs(50, 1000, 0.3)
    idx = np.arange(1000)
    first = _raw(src, tgt, idx, idx, max_trials=20000, confidence=0.0)
    cloud = np.concatenate([src, tgt])
    for _ in range(3):
        again = _raw(src, tgt, idx, idx, max_trials=20000, confidence=0.0)
        assert again[0] == 0 and np.array_equal(again[2], first[2])
        _same(again[1], first[1])
        fi.segment_plane(cloud, 0.1)
        fi.register_points(src[:200], tgt, mode="point", max_iterations=2)


def test_error_codes(fi):
    src, tgt = lattice_pairs()
    idx = np.arange(64)
    INVALID, UNSUPPORTED = 1, 5
    bad = [dict(threshold=-1.0), dict(threshold=math.nan), dict(similarity=-0.1), dict(similarity=1.5), dict(similarity=math.nan),
           dict(confidence=1.0), dict(confidence=-0.5), dict(confidence=math.nan), dict(max_trials=0), dict(max_trials=2 ** 31),
           dict(memory=2), dict(ps=None), dict(pt=None), dict(psi=None), dict(pti=None), dict(opt=None), dict(out=None),
           dict(m=-1), dict(ns=-1), dict(nt=-1)]
    for kw in bad:
        assert _raw(src, tgt, idx, idx, **kw)[0] == INVALID, kw
    for kw in (dict(m=2 ** 31), dict(ns=2 ** 31), dict(nt=2 ** 31)):
        assert _raw(src, tgt, idx, idx, **kw)[0] == UNSUPPORTED, kw
    from field_interpolation_amd import _capi
    assert b"pairs" in _capi.lib().fi_last_error()
    assert _raw(src, tgt, idx, idx, inl=None)[0] == 0                                    # inliers may be NULL
    assert _raw(src, tgt, idx, idx, max_trials=2 ** 31 - 1, confidence=0.5)[0] == 0       # (stops after the first batch)
    assert _raw(src, tgt, idx[:0], idx[:0], ps=None, pt=None, ns=0, nt=0)[0] == 0          # nothing at all
    code, res, _ = _raw(src[:0], tgt, idx, idx)                                          # no source point: no pair is live
    assert code == 0 and (res["found"], res["pairs"], res["live"]) == (False, 64, 0)
    with pytest.raises(_capi.FiError):
        fi.align_correspondences(src, tgt, idx, idx, -1.0)
    with pytest.raises(ValueError):
        fi.align_correspondences(src[:, :2], tgt, idx, idx, 0.1)
    with pytest.raises(ValueError):
        fi.align_correspondences(src, tgt, idx, idx[:5], 0.1)


def test_device_tensors(tmp_path, planted):
    """the same answers from torch tensors that stay on the device, checked in a fresh process (tests/align_torch_worker.py),
    as torch must stay out of this one"""
    p = planted
    np.savez(tmp_path / "in.npz", sp=p["sp"], sn=p["sn"], tp=p["tp"], tn=p["tn"])
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "align_torch_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    o = np.load(tmp_path / "out.npz")
    assert o["on_device"].all()
    fs, vs = FR.describe(p["sp"], p["sn"], 32)
    ft, vt = FR.describe(p["tp"], p["tn"], 32)
    assert np.array_equal(o["features"].view(np.uint32), fs.view(np.uint32)) and np.array_equal(o["valid"], vs.astype(bool))
    assert np.array_equal(o["matches"], p["matches"]) and np.array_equal(o["mutual"], p["mutual"])
    assert _bits(o["distances"].astype(np.float64)) == _bits(FR.match(fs, ft, vs, vt)[1].astype(np.float64))
    want, want_inl = AR.align(p["sp"], p["tp"], np.arange(len(p["sp"])), p["matches"], 1.0, max_trials=16384, confidence=0.0)
    assert o["ints"].tolist() == [int(want[k]) for k in INTS] and np.array_equal(o["mask"], want_inl.astype(bool))
    assert _bits(o["doubles"]) == _bits(list(want["transform"].ravel()) + [want["rms"]])
    ref = RR.register(RR.Target(points=p["tp"], normals=p["tn"]), p["sp"], max_distance=3.0, initial=want["transform"])
    assert _bits(o["refined"]) == _bits(ref["transform"])
