"""The moving-least-squares kernels (fi_mls.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_mls.usage.txt): every kernel instance is there, none has VGPR or SGPR spills, scratch, AGPRs or
LDS, the walk keeps k_cloud_neighbours' occupancy floors of 8 / 8 / 5 waves per SIMD at the capacities 8 / 16 / 32 (it holds
no sorted slot in its list, which is what that costs), and the fit stays within DESIGN.md 4.25's table."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")

# DESIGN.md 4.25's table: what hipcc reports for gfx950, rounded up to the next multiple of 8 (the larger of the two instances
# over whose points the queries are).  The walk by capacity (the larger of 2-D and 3-D), the fit by (dimension, degree):
# (VGPRs, waves per SIMD)
WALK = {8: 48, 16: 64, 32: 96}
WALK_OCCUPANCY = {8: 8, 16: 8, 32: 5}
FIT = {(2, 1): (48, 8), (2, 2): (72, 7), (3, 1): (64, 8), (3, 2): (128, 4)}
SMALL = {"k_mls_slots": 8, "k_mls_rest": 16}


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_mls.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_mls_" in k}


def _walk(name):
    """the template arguments (D, CAP, SELF) of a mangled k_mls_walk"""
    m = re.search(r"k_mls_walkILi(\d+)ELi(\d+)ELb([01])E", name)
    return (int(m.group(1)), int(m.group(2)), int(m.group(3))) if m else None


def _fit(name):
    """the template arguments (D, DEG, SELF) of a mangled k_mls_fit"""
    m = re.search(r"k_mls_fitILi(\d+)ELi(\d+)ELb([01])E", name)
    return (int(m.group(1)), int(m.group(2)), int(m.group(3))) if m else None


def test_every_instance_is_there_and_none_spills_or_uses_scratch_agprs_or_lds():
    rep = _report()
    assert sorted(_walk(k) for k in rep if _walk(k)) == [(d, c, s) for d in (2, 3) for c in (8, 16, 32) for s in (0, 1)]
    assert sorted(_fit(k) for k in rep if _fit(k)) == [(d, g, s) for d in (2, 3) for g in (1, 2) for s in (0, 1)]
    assert sum(1 for k in rep if "k_mls_slots" in k) == 1 and sum(1 for k in rep if "k_mls_rest" in k) == 1
    assert len(rep) == 12 + 8 + 2, sorted(rep)
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] == 0, name


def test_the_walk_keeps_the_neighbour_walks_waves():
    for name, r in _report().items():
        if _walk(name):
            cap = _walk(name)[1]
            assert r["Occupancy [waves/SIMD]"] >= WALK_OCCUPANCY[cap], (name, r["Occupancy [waves/SIMD]"])
            assert r["VGPRs"] <= WALK[cap], (name, r["VGPRs"])


def test_the_fit_keeps_what_the_design_states():
    for name, r in _report().items():
        if _fit(name):
            vgprs, waves = FIT[_fit(name)[:2]]
            assert r["VGPRs"] <= vgprs, (name, r["VGPRs"])
            assert r["Occupancy [waves/SIMD]"] >= waves, (name, r["Occupancy [waves/SIMD]"])
        elif not _walk(name):
            budget = [v for k, v in SMALL.items() if k in name][0]
            assert r["VGPRs"] <= budget and r["Occupancy [waves/SIMD]"] >= 8, (name, r)
