"""The k-nearest-point and normal kernels (fi_knn.hip) against the compiler's resource report the build keeps next to the
object (field_interpolation_amd/csrc/fi_knn.usage.txt): no VGPR or SGPR spills, no scratch (the neighbour lists live in
registers), no AGPRs, and the query classes up to k = 16 within 64 VGPRs."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_knn.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_knn_" in k}


def _class(name, kernel):
    """the template arguments (D, CAP) of a mangled k_knn_query / k_knn_normals"""
    m = re.search(kernel + r"ILi(\d+)ELi(\d+)E", name)
    return int(m.group(1)), int(m.group(2))


def test_knn_kernels_spill_nothing_and_use_no_scratch_or_agprs():
    rep = _report()
    # the queries (1-, 2- and 3-D x the classes 8, 16, 32), the normals (2- and 3-D x the classes), the blank fill
    assert len(rep) == 9 + 6 + 1, sorted(rep)
    assert sum("k_knn_query" in k for k in rep) == 9 and sum("k_knn_normals" in k for k in rep) == 6
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] == 0, name


def test_query_classes_up_to_sixteen_keep_eight_waves():
    # the walk is latency-bound: 64 VGPRs are 8 waves per SIMD; the class of 32 holds 64 registers of pairs alone
    rep = {k: v for k, v in _report().items() if "k_knn_query" in k}
    classes = sorted(_class(k, "k_knn_query") for k in rep)
    assert classes == [(d, c) for d in (1, 2, 3) for c in (8, 16, 32)]
    for name, r in rep.items():
        if _class(name, "k_knn_query")[1] <= 16:
            assert r["VGPRs"] <= 64, (name, r["VGPRs"])
        else:
            assert r["VGPRs"] <= 128, (name, r["VGPRs"])        # 4 waves at least


def test_normal_kernels_keep_what_the_design_states():
    # DESIGN.md 4.11's table: the fused kernels carry a third register per pair (the slot) and the fp64 fit
    rep = {k: v for k, v in _report().items() if "k_knn_normals" in k}
    budget = {8: 64, 16: 96, 32: 168}
    for name, r in rep.items():
        assert r["VGPRs"] <= budget[_class(name, "k_knn_normals")[1]], (name, r["VGPRs"])
