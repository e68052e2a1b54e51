"""The colour kernels (fi_colour.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_colour.usage.txt): every kernel instance is there, none has VGPR or SGPR spills, scratch,
AGPRs or LDS, each stays within DESIGN.md 4.29's table, and every one within the 64 VGPRs of 8 waves per SIMD."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")

# DESIGN.md 4.29's table: what hipcc reports for gfx950, rounded up to the next multiple of 8: (VGPRs, waves per SIMD).  The
# template arguments as the mangled names spell them: ILi<C>ELb<wide load>EE for k_colour_integrate, ILi<C>EE for k_colour_sample.
BUDGET = {"k_colour_integrateILi1ELb0EE": (40, 8), "k_colour_integrateILi2ELb0EE": (40, 8), "k_colour_integrateILi2ELb1EE": (40, 8),
          "k_colour_integrateILi3ELb0EE": (40, 8), "k_colour_integrateILi4ELb0EE": (48, 8), "k_colour_integrateILi4ELb1EE": (48, 8),
          "k_colour_sampleILi1EE": (32, 8), "k_colour_sampleILi2EE": (32, 8), "k_colour_sampleILi3EE": (40, 8),
          "k_colour_sampleILi4EE": (40, 8), "k_colour_mark": (8, 8), "k_colour_gather": (24, 8)}


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_colour.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_colour_" in k}


def _kernel(name):
    return [k for k in BUDGET if k in name][0]


def test_every_instance_is_there_and_none_spills_or_uses_scratch_agprs_or_lds():
    rep = _report()
    assert sorted(_kernel(k) for k in rep) == sorted(BUDGET), sorted(rep)
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] == 0, name


def test_the_kernels_keep_what_the_design_states():
    for name, r in _report().items():
        vgprs, waves = BUDGET[_kernel(name)]
        assert vgprs <= 64
        assert r["VGPRs"] <= vgprs, (name, r["VGPRs"])
        assert r["Occupancy [waves/SIMD]"] >= waves, (name, r["Occupancy [waves/SIMD]"])
