"""The mesh-smoothing kernels (fi_smooth.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_smooth.usage.txt): no VGPR or SGPR spills, no scratch, no AGPRs, no LDS, and the register
counts DESIGN.md 4.16 states.  Every kernel is gather- or sort-bound and stays far below the 64 VGPRs of 8 waves per SIMD;
the step kernel, the hot path, carries two fp64 vectors and needs 30 at the most."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")

# DESIGN.md 4.16's table (the larger of 2-D / 3-D where a kernel is a template), each with the margin the neighbouring
# resource tests leave for a compiler update
BUDGET = {"k_smooth_finite": 16, "k_smooth_pairs": 32, "k_smooth_boundary": 16, "k_smooth_flags": 24, "k_smooth_compact": 16,
          "k_smooth_starts": 24, "k_smooth_widen": 16, "k_smooth_step": 40, "k_smooth_incidence": 24, "k_smooth_normals": 40}
# how many instances of each the unit holds: templates over D (and the step over clamp and cast)
INSTANCES = {"k_smooth_finite": 2, "k_smooth_pairs": 2, "k_smooth_boundary": 2, "k_smooth_flags": 2, "k_smooth_compact": 1,
             "k_smooth_starts": 1, "k_smooth_widen": 1, "k_smooth_step": 8, "k_smooth_incidence": 2, "k_smooth_normals": 2}


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_smooth.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_smooth_" in k}


def _kernel(name):
    return re.search(r"k_smooth_[a-z_]+?(?=I|E)", name).group(0)


def test_smooth_kernels_spill_nothing_and_use_no_scratch_agprs_or_lds():
    rep = _report()
    names = sorted(_kernel(k) for k in rep)
    assert names == sorted(k for k, n in INSTANCES.items() for _ in range(n)), names
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] == 0, name


def test_smooth_kernels_keep_what_the_design_states():
    for name, r in _report().items():
        assert r["VGPRs"] <= BUDGET[_kernel(name)], (name, r["VGPRs"])
        assert r["Occupancy [waves/SIMD]"] == 8, name
