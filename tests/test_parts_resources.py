"""The mesh-parts kernels (fi_parts.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_parts.usage.txt): no VGPR or SGPR spills, no scratch, no AGPRs, and the register counts
DESIGN.md 4.13 states -- the kernels are gather-, atomic- and sort-bound, so every one of them stays at or below the 64 VGPRs
of 8 waves per SIMD.  Only the measuring pass uses LDS (its four waves' partial sums and boxes)."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")

# DESIGN.md 4.13's table (2-D / 3-D where a kernel is a template), each with the margin the neighbouring resource tests
# leave for a compiler update
BUDGET = {"k_parts_start": 16, "k_parts_union": 24, "k_parts_jump": 16, "k_parts_roots": 16, "k_parts_label_vertices": 16,
          "k_parts_label_prims": 16, "k_parts_check": 16, "k_parts_iota": 16, "k_parts_halfedges": 24, "k_parts_classify": 24,
          "k_parts_degrees": 24, "k_parts_count_prims": 16, "k_parts_count_vertices": 24, "k_parts_sort_keys": 16,
          "k_parts_first": 16, "k_parts_chunk_counts": 16, "k_parts_chunks": 64, "k_parts_rows": 40, "k_parts_keep_flags": 16,
          "k_parts_gather_vertices": 24, "k_parts_gather_prims": 24}
TEMPLATES = {"k_parts_union", "k_parts_label_prims", "k_parts_chunks", "k_parts_gather_vertices", "k_parts_gather_prims"}
LDS = {"k_parts_chunks": 160}


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_parts.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_parts_" in k}


def _kernel(name):
    return re.search(r"k_parts_[a-z_]+?(?=I|E)", name).group(0)


def test_parts_kernels_spill_nothing_and_use_no_scratch_or_agprs():
    rep = _report()
    names = sorted(_kernel(k) for k in rep)
    assert len(names) == 26
    assert names == sorted([k for k in BUDGET if k not in TEMPLATES] + 2 * sorted(TEMPLATES)), names
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] == LDS.get(_kernel(name), 0), name


def test_parts_kernels_keep_what_the_design_states():
    for name, r in _report().items():
        assert r["VGPRs"] <= BUDGET[_kernel(name)], (name, r["VGPRs"])
        assert r["Occupancy [waves/SIMD]"] == 8, name
