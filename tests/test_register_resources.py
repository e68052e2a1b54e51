"""The registration kernels (fi_register.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_register.usage.txt): every kernel is there, none has VGPR or SGPR spills, scratch or AGPRs,
and LDS and registers stay within what DESIGN.md 4.18's table states.  k_reg_pairs, the hot path, carries the 29 sums of a
3-D step as doubles (58 registers) next to the pair it forms; its LDS is eight sums of half a block at a time, not all 29."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")

# DESIGN.md 4.18's table (the largest instance where a kernel is a template), each with the margin the neighbouring resource
# tests leave for a compiler update
BUDGET = {"k_reg_bounds": 24, "k_reg_init": 32, "k_reg_transform": 24, "k_reg_unsort": 8, "k_reg_pairs": 128, "k_reg_finish": 64}
# how many instances of each the unit holds: templates over D (the pairs also over the mode and the kind of target)
INSTANCES = {"k_reg_bounds": 2, "k_reg_init": 2, "k_reg_transform": 2, "k_reg_unsort": 2, "k_reg_pairs": 8, "k_reg_finish": 2}
# bytes a block: the pairs' eight sums of 128 doubles and the four waves' counts; the step's small matrices (3-D)
LDS = {"k_reg_pairs": 8 * 128 * 8 + 4 * 4 * 4, "k_reg_finish": 1024}
# waves a SIMD at the least: the 3-D pairs hold 58 registers of sums
OCCUPANCY = {"k_reg_pairs": 4}


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_register.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_reg_" in k}


def _kernel(name):
    return re.search(r"k_reg_[a-z_]+?(?=I|E)", name).group(0)


def test_register_kernels_spill_nothing_and_use_no_scratch_or_agprs():
    rep = _report()
    names = sorted(_kernel(k) for k in rep)
    assert names == sorted(k for k, n in INSTANCES.items() for _ in range(n)), names
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] <= LDS.get(_kernel(name), 0), name


def test_register_kernels_keep_what_the_design_states():
    for name, r in _report().items():
        assert r["VGPRs"] <= BUDGET[_kernel(name)], (name, r["VGPRs"])
        assert r["Occupancy [waves/SIMD]"] >= OCCUPANCY.get(_kernel(name), 8), name
