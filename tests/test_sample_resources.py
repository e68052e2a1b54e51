"""The point-query kernels (fi_sample.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_sample.usage.txt): no VGPR or SGPR spills, no scratch, no AGPRs."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_sample.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def test_sample_kernels_have_no_spills_scratch_or_agprs():
    rep = {k: v for k, v in _report().items() if "k_sample" in k}
    # 1-, 2- and 3-D x linear / cubic x fp32 / fp64 x with / without gradients; the slab fill (1-3 D) and the group sum
    assert len(rep) == 24 + 3 + 1, sorted(rep)
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name


def test_linear_kernels_keep_eight_waves():
    # the gather is latency-bound: the linear kernels stay within 64 VGPRs (8 waves per SIMD)
    rep = {k: v for k, v in _report().items() if re.search(r"k_sample.*ILi\dELi0E", k)}
    assert len(rep) == 12, sorted(rep)
    for name, r in rep.items():
        assert r["VGPRs"] <= 64, (name, r["VGPRs"])
