"""The nearest-point kernels (fi_nearest.hip, and the shared build kernels of fi_bvh.h as this unit instantiates them) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_nearest.usage.txt): no VGPR or SGPR spills, no scratch, no AGPRs."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_nearest.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def test_nearest_kernels_spill_nothing_and_use_no_scratch_or_agprs():
    rep = {k: v for k, v in _report().items() if "k_nearest" in k or "k_bvh_" in k}
    # the queries (k_nearest_query): 1-, 2- and 3-D x (a query buffer, the lattice, the border list); the build (k_bvh_*):
    # bounds (1-3 D) and their total, Morton codes (1-3 D), the gather (1-3 D), the leaf boxes (1-3 D), the node boxes
    assert len(rep) == 9 + 3 + 1 + 3 + 3 + 3 + 1, sorted(rep)
    assert sum("k_bvh_" in k for k in rep) == 3 + 1 + 3 + 3 + 3 + 1, sorted(rep)
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name


def test_query_kernels_keep_eight_waves():
    # the walk is latency-bound: the query kernels stay within 64 VGPRs (8 waves per SIMD) and use no LDS
    rep = {k: v for k, v in _report().items() if "k_nearest_query" in k}
    assert len(rep) == 9, sorted(rep)
    for name, r in rep.items():
        assert r["VGPRs"] <= 64, (name, r["VGPRs"])
        assert r["LDS Size [bytes/block]"] == 0, name
