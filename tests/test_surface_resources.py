"""The surface-distance kernels (fi_surface.hip, and the shared build kernels of fi_bvh.h as this unit instantiates them) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_surface.usage.txt): no VGPR or SGPR spills, no scratch, no AGPRs; the query kernels use
no LDS and keep the occupancy DESIGN.md 4.9 records."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_surface.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def test_surface_kernels_spill_nothing_and_use_no_scratch_or_agprs():
    rep = {k: v for k, v in _report().items() if "k_surf_" in k or "k_bvh_" in k}
    # the queries (k_surf_query): 2- and 3-D x (a query buffer, the lattice, the signed lattice); the build (k_bvh_*): bounds
    # (2-3 D) and their total, Morton codes (2-3 D), the gather (2-3 D), the leaf boxes (2-3 D), the node boxes
    assert len(rep) == 6 + 2 + 1 + 2 + 2 + 2 + 1, sorted(rep)
    assert sum("k_bvh_" in k for k in rep) == 2 + 1 + 2 + 2 + 2 + 1, sorted(rep)
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name


def test_query_kernels_use_no_lds_and_keep_their_occupancy():
    # 2-D: within 64 VGPRs (8 waves per SIMD); 3-D: Ericson's test holds 70 (7 waves: 8 would spill), DESIGN.md 4.9
    rep = {k: v for k, v in _report().items() if "k_surf_query" in k}
    assert len(rep) == 6, sorted(rep)
    for name, r in rep.items():
        assert r["LDS Size [bytes/block]"] == 0, name
        waves = 8 if "ILi2E" in name else 7
        assert r["Occupancy [waves/SIMD]"] >= waves, (name, r["Occupancy [waves/SIMD]"])
        assert r["VGPRs"] <= 512 // waves // 8 * 8, (name, r["VGPRs"])
