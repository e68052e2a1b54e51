"""The ray kernels (fi_ray.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_ray.usage.txt): no VGPR or SGPR spills, no scratch, no AGPRs, no LDS, and the occupancy
DESIGN.md 4.14 records."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_ray.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_ray_" in k}


def test_ray_kernels_spill_nothing_and_use_no_scratch_or_agprs():
    rep = _report()
    # the closest hit (k_ray_hit): 2- and 3-D; the counts (k_ray_count): 2- and 3-D x (counts, containment, the sign of
    # queried points, the sign of a lattice)
    assert len(rep) == 2 + 8, sorted(rep)
    assert sum("k_ray_hit" in k for k in rep) == 2 and sum("k_ray_count" in k for k in rep) == 8, sorted(rep)
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name


def test_ray_kernels_use_no_lds_and_keep_their_occupancy():
    # every kernel within 64 VGPRs: 8 waves per SIMD (3-D: 54 for the closest hit, 46 for the counts; 2-D: 42 and 34)
    for name, r in _report().items():
        assert r["LDS Size [bytes/block]"] == 0, name
        assert r["Occupancy [waves/SIMD]"] == 8, (name, r["Occupancy [waves/SIMD]"])
        assert r["VGPRs"] <= 64, (name, r["VGPRs"])
