"""The descriptor and matching kernels (fi_feature.hip) against the compiler's resource report the build keeps next to the
object (field_interpolation_amd/csrc/fi_feature.usage.txt): every kernel instance is there, none has VGPR or SGPR spills,
scratch or AGPRs -- the packed counters of k_feat_spfh and the 33 accumulators of k_feat_fpfh stay in registers --, LDS is
what a tile of 256 rows needs, and registers and occupancy stay within DESIGN.md 4.22's table."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")

# DESIGN.md 4.22's table: what hipcc reports for gfx950, rounded up to the next multiple of 8; k_feat_match by padded width
BUDGET = {"k_feat_positions": 16, "k_feat_live": 24, "k_feat_spfh": 80, "k_feat_fpfh": 144, "k_feat_match_out": 8}
MATCH = {8: 40, 16: 56, 32: 72, 40: 112, 64: 136}
# waves per SIMD: the two descriptor kernels hold a pair's frame or the 33 accumulators in fp64; k_feat_match is bound by its
# LDS tile (256 rows of the padded width in fp32), which also caps the workgroups a CU holds
OCCUPANCY = {"k_feat_spfh": 6, "k_feat_fpfh": 3}
MATCH_OCCUPANCY = {8: 8, 16: 8, 32: 5, 40: 4, 64: 2}


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_feature.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_feat_" in k}


def _kernel(name):
    """(kernel, padded width or None)"""
    m = re.search(r"\d+k_feat_matchILi(\d+)E", name)
    if m:
        return "k_feat_match", int(m.group(1))
    return re.search(r"\d+(k_feat_[a-z_]+?)(?=I|E)", name).group(1), None


def test_feature_kernels_spill_nothing_and_use_no_scratch_or_agprs():
    rep = _report()
    names = sorted(_kernel(k) for k in rep if _kernel(k)[1] is None)
    assert [n for n, _ in names] == sorted(BUDGET), names
    assert sorted(_kernel(k)[1] for k in rep if _kernel(k)[1] is not None) == sorted(MATCH)
    for name, r in rep.items():
        kernel, width = _kernel(name)
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] == (256 * width * 4 if width else 0), name


def test_feature_kernels_keep_what_the_design_states():
    for name, r in _report().items():
        kernel, width = _kernel(name)
        assert r["VGPRs"] <= (MATCH[width] if width else BUDGET[kernel]), (name, r["VGPRs"])
        assert r["Occupancy [waves/SIMD]"] >= (MATCH_OCCUPANCY[width] if width else OCCUPANCY.get(kernel, 8)), name
