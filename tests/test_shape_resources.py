"""The sphere and cylinder kernels (fi_shape.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_shape.usage.txt): every kernel instance is there, none has VGPR or SGPR spills, scratch or
AGPRs, LDS is what the tiles and the tree sums need, and registers and occupancy stay within DESIGN.md 4.26's table."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")

# DESIGN.md 4.26's table: what hipcc reports for gfx950, rounded up to the next multiple of 8 (the largest instance where a
# kernel is a template over the model, the dimension or the pass; the score by instance below)
BUDGET = {"k_shape_cand": 16, "k_shape_models": 64, "k_shape_keys": 16, "k_shape_pick": 48, "k_shape_flags": 48, "k_shape_chunks": 40,
          "k_shape_finish": 72, "k_shape_label": 8}
# the score by (model, dimension, normals staged): (VGPRs, waves per SIMD).  The sphere without normals is the plane's kernel
# with three subtractions more: the same 72 registers and 7 waves.  The cylinder keeps eight points' loads and 21 fp64
# operations a point in flight in 104 registers, 4 waves: its loop is bound by fp64 issue, which 4 waves of eight independent
# points each keep busy (profiles/shape.md)
SCORE = {(0, 3, 0): (72, 7), (0, 3, 1): (56, 8), (0, 2, 0): (56, 8), (0, 2, 1): (48, 8), (1, 3, 0): (104, 4), (1, 3, 1): (64, 8)}
# how many instances of each the unit holds: the sphere in 2-D and 3-D and the cylinder; the score with and without staged
# normals; the chunk sums and their finish over three passes; the candidates by the dimension alone
INSTANCES = {"k_shape_cand": 2, "k_shape_models": 3, "k_shape_score": 6, "k_shape_keys": 1, "k_shape_pick": 3, "k_shape_flags": 3,
             "k_shape_chunks": 9, "k_shape_finish": 9, "k_shape_label": 1}
# bytes a block: a tile of 256 staged points of 8 doubles (3-D with normals; 4 without, half of either in 2-D); the tree over
# 256 doubles for each of up to 10 sums
LDS = {"k_shape_score": 256 * 8 * 8, "k_shape_chunks": 10 * 256 * 8}
# waves per SIMD below 8: the finish of a 3-D sphere's Kasa pass is one wave that holds ten totals and a 3 x 3 solve
OCCUPANCY = {"k_shape_finish": 7}


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_shape.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_shape_" in k}


def _kernel(name):
    return re.search(r"\d+(k_shape_[a-z_]+?)(?=I|E)", name).group(1)


def _score_instance(name):
    m = re.search(r"k_shape_scoreILi(\d)ELi(\d)ELb(\d)E", name)
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def test_shape_kernels_spill_nothing_and_use_no_scratch_or_agprs():
    rep = _report()
    names = sorted(_kernel(k) for k in rep)
    assert names == sorted(k for k, n in INSTANCES.items() for _ in range(n)), names
    assert sorted(_score_instance(k) for k in rep if _kernel(k) == "k_shape_score") == sorted(SCORE)
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] <= LDS.get(_kernel(name), 0), name


def test_shape_kernels_keep_what_the_design_states():
    for name, r in _report().items():
        kernel = _kernel(name)
        vgprs, waves = SCORE[_score_instance(name)] if kernel == "k_shape_score" else (BUDGET[kernel], OCCUPANCY.get(kernel, 8))
        assert r["VGPRs"] <= vgprs, (name, r["VGPRs"])
        assert r["Occupancy [waves/SIMD]"] >= waves, name
