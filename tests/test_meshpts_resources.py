"""The mesh sampling / deviation kernels (fi_meshpts.hip) against the compiler's resource report the build keeps next to the
object (field_interpolation_amd/csrc/fi_meshpts.usage.txt): no VGPR or SGPR spills, no scratch, no AGPRs, LDS only in the
reduction kernel (two arrays of 256 eight-byte words), 8 waves per SIMD everywhere, and the register counts DESIGN.md 4.17
states.  The sampler, the hot path, carries a triangle's nine fp64 coordinates and needs 48 at the most (3-D, vertex normals)."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")

# DESIGN.md 4.17's table (the largest instance where a kernel is a template), each with the margin the neighbouring resource
# tests leave for a compiler update
BUDGET = {"k_mpts_weight": 32, "k_mpts_max": 16, "k_mpts_q": 16, "k_mpts_sample": 56, "k_mpts_mark": 16, "k_mpts_compact": 16,
          "k_mpts_scatter": 16, "k_mpts_reduce": 24, "k_mpts_finish": 24}
# how many instances of each the unit holds: templates over D (and the sampler over the normals it writes)
INSTANCES = {"k_mpts_weight": 2, "k_mpts_max": 1, "k_mpts_q": 1, "k_mpts_sample": 6, "k_mpts_mark": 1, "k_mpts_compact": 2,
             "k_mpts_scatter": 1, "k_mpts_reduce": 1, "k_mpts_finish": 1}
LDS = {"k_mpts_reduce": 2 * 256 * 8}


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_meshpts.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_mpts_" in k}


def _kernel(name):
    return re.search(r"k_mpts_[a-z_]+?(?=I|E)", name).group(0)


def test_meshpts_kernels_spill_nothing_and_use_no_scratch_or_agprs():
    rep = _report()
    names = sorted(_kernel(k) for k in rep)
    assert names == sorted(k for k, n in INSTANCES.items() for _ in range(n)), names
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] == LDS.get(_kernel(name), 0), name


def test_meshpts_kernels_keep_what_the_design_states():
    for name, r in _report().items():
        assert r["VGPRs"] <= BUDGET[_kernel(name)], (name, r["VGPRs"])
        assert r["Occupancy [waves/SIMD]"] == 8, name
