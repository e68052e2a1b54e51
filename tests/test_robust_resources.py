"""The robust-fit kernels (fi_robust.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_robust.usage.txt): no VGPR or SGPR spills, no scratch, no AGPRs in any kernel of the file;
the residual kernels -- latency-bound gathers -- within 64 VGPRs (8 waves per SIMD)."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_robust.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def test_no_kernel_of_the_file_spills_or_uses_scratch_or_agprs():
    rep = _report()
    own = {k: v for k, v in rep.items() if re.search(r"k_point_residual|k_pick_scale|k_robust_weights|k_fill_ones", k)}
    # the residual pass in 1, 2 and 3-D x fp32 / fp64; the scale pick, the weight pass, the fill of ones
    assert len(own) == 6 + 3, sorted(own)
    assert len(rep) > len(own)          # (the sort's kernels and the shared helpers are in the report too)
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name


def test_residual_kernels_keep_eight_waves():
    rep = {k: v for k, v in _report().items() if "k_point_residual" in k}
    assert len(rep) == 6, sorted(rep)
    for name, r in rep.items():
        assert r["VGPRs"] <= 64, (name, r["VGPRs"])
