"""The mesh-simplification kernels (fi_simplify.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_simplify.usage.txt): no VGPR or SGPR spills, no scratch, no AGPRs, no LDS, and the register
counts DESIGN.md 4.15 states.  Every kernel but one is gather- and sort-bound and stays far below the 64 VGPRs of 8 waves per
SIMD; the 3-D quadric placement carries A, V, b, the mean and the cell centre in fp64 through the Jacobi iteration and runs at
5 waves per SIMD (at most 96 VGPRs)."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")

# DESIGN.md 4.15's table (the larger of 2-D / 3-D where a kernel is a template), each with the margin the neighbouring
# resource tests leave for a compiler update
BUDGET = {"k_simp_mark": 16, "k_simp_keys": 24, "k_simp_heads": 16, "k_simp_assign": 24, "k_simp_tuple_low": 24,
          "k_simp_tuple_high": 24, "k_simp_keep": 24, "k_simp_cluster_flags": 24, "k_simp_pairs": 24, "k_simp_pair_first": 16,
          "k_simp_gather_vertices": 24, "k_simp_gather_prims": 24, "k_simp_vertex_map": 16}
# k_simp_place<D, QUADRIC>: (VGPR budget, waves per SIMD)
PLACE = {"ILi2ELb0E": (40, 8), "ILi2ELb1E": (64, 8), "ILi3ELb0E": (48, 8), "ILi3ELb1E": (96, 5)}
TEMPLATES = {"k_simp_keys", "k_simp_tuple_low", "k_simp_tuple_high", "k_simp_keep", "k_simp_cluster_flags", "k_simp_pairs",
             "k_simp_gather_vertices", "k_simp_gather_prims"}


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_simplify.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_simp_" in k}


def _kernel(name):
    return re.search(r"k_simp_[a-z_]+?(?=I|E)", name).group(0)


def test_simplify_kernels_spill_nothing_and_use_no_scratch_agprs_or_lds():
    rep = _report()
    names = sorted(_kernel(k) for k in rep)
    assert names == sorted([k for k in BUDGET if k not in TEMPLATES] + 2 * sorted(TEMPLATES) + 4 * ["k_simp_place"]), names
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] == 0, name


def test_simplify_kernels_keep_what_the_design_states():
    seen = set()
    for name, r in _report().items():
        if _kernel(name) == "k_simp_place":
            variant = re.search(r"k_simp_place(ILi\dELb\dE)", name).group(1)
            seen.add(variant)
            budget, waves = PLACE[variant]
        else:
            budget, waves = BUDGET[_kernel(name)], 8
        assert r["VGPRs"] <= budget, (name, r["VGPRs"])
        assert r["Occupancy [waves/SIMD]"] == waves, name
    assert seen == set(PLACE)
