"""The alignment kernels (fi_align.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_align.usage.txt): every kernel is there, none has VGPR or SGPR spills, scratch or AGPRs, LDS
is what the tile and the tree sum need, and registers and occupancy stay within DESIGN.md 4.22's table."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")

# DESIGN.md 4.22's table: what hipcc reports for gfx950, rounded up to the next multiple of 8
BUDGET = {"k_align_live": 8, "k_align_models": 96, "k_align_score": 120, "k_align_keys": 16, "k_align_pick": 88, "k_align_flags": 24,
          "k_align_chunks": 32, "k_align_finish": 24}
# bytes a block: a tile of 256 staged pairs of 6 doubles; the tree over 256 doubles
LDS = {"k_align_score": 256 * 6 * 8, "k_align_chunks": 256 * 8}
# waves per SIMD: a hypothesis is two frames and a 3 x 3 product in fp64, the score keeps 12 doubles a lane and four pairs'
# loads in flight; both are bound by arithmetic and LDS reads, not by occupancy
OCCUPANCY = {"k_align_models": 5, "k_align_score": 4, "k_align_pick": 5}


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_align.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_align_" in k}


def _kernel(name):
    return re.search(r"\d+(k_align_[a-z_]+?)(?=I|E)", name).group(1)


def test_align_kernels_spill_nothing_and_use_no_scratch_or_agprs():
    rep = _report()
    assert sorted(_kernel(k) for k in rep) == sorted(BUDGET), sorted(rep)
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] == LDS.get(_kernel(name), 0), name


def test_align_kernels_keep_what_the_design_states():
    for name, r in _report().items():
        assert r["VGPRs"] <= BUDGET[_kernel(name)], (name, r["VGPRs"])
        assert r["Occupancy [waves/SIMD]"] >= OCCUPANCY.get(_kernel(name), 8), name
