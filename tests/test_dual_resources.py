"""The dual-contouring kernels (fi_dual.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_dual.usage.txt): no VGPR or SGPR spills, no scratch, no AGPRs."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_dual.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def test_dual_kernels_have_no_spills_scratch_or_agprs():
    rep = {k: v for k, v in _report().items() if "k_dc_" in k}
    # count / compact / emit for 2-D and 3-D, and the totals kernel
    assert len(rep) == 7, sorted(rep)
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
