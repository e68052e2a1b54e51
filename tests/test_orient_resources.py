"""The orientation kernels (fi_orient.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_orient.usage.txt): no VGPR or SGPR spills, no scratch, no AGPRs, no LDS, and the register
counts DESIGN.md 4.12 states -- the kernels are gather- and atomic-bound, so every one of them stays far below the 64 VGPRs
of 8 waves per SIMD."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")

# DESIGN.md 4.12's table (2-D / 3-D where a kernel is a template), each with the margin the neighbouring resource tests
# leave for a compiler update
BUDGET = {"k_orient_positions": 16, "k_orient_start": 24, "k_orient_edges": 24, "k_orient_propose": 24, "k_orient_select": 24,
          "k_orient_hook": 32, "k_orient_jump": 16, "k_orient_collect": 32, "k_orient_decide": 24, "k_orient_apply": 16}
TEMPLATES = {"k_orient_positions", "k_orient_start", "k_orient_edges", "k_orient_hook", "k_orient_collect", "k_orient_decide",
             "k_orient_apply"}


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_orient.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_orient_" in k}


def _kernel(name):
    return re.search(r"k_orient_[a-z]+", name).group(0)


def test_orient_kernels_spill_nothing_and_use_no_scratch_agprs_or_lds():
    rep = _report()
    names = sorted(_kernel(k) for k in rep)
    assert names == sorted([k for k in BUDGET if k not in TEMPLATES] + 2 * sorted(TEMPLATES)), names
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] == 0, name


def test_orient_kernels_keep_what_the_design_states():
    for name, r in _report().items():
        assert r["VGPRs"] <= BUDGET[_kernel(name)], (name, r["VGPRs"])
