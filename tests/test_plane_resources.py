"""The plane kernels (fi_plane.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_plane.usage.txt): every kernel instance is there, none has VGPR or SGPR spills, scratch or
AGPRs, LDS is what the tiles and the tree sums need, and registers and occupancy stay within DESIGN.md 4.21's table."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")

# DESIGN.md 4.21's table: what hipcc reports for gfx950, rounded up to the next multiple of 8 (the largest instance where a
# kernel is a template over the dimension or the pass)
BUDGET = {"k_plane_cand": 8, "k_plane_models": 32, "k_plane_score": 72, "k_plane_keys": 16, "k_plane_pick": 24, "k_plane_flags": 8,
          "k_plane_chunks": 24, "k_plane_finish": 56, "k_plane_label": 8}
# how many instances of each the unit holds: D = 2, 3; the chunk sums and their finish over three passes as well
INSTANCES = {"k_plane_cand": 2, "k_plane_models": 2, "k_plane_score": 2, "k_plane_keys": 1, "k_plane_pick": 2, "k_plane_flags": 2,
             "k_plane_chunks": 6, "k_plane_finish": 6, "k_plane_label": 1}
# bytes a block: a tile of 256 staged points of 4 doubles (3-D; 2 in 2-D); the tree over 256 doubles for each of up to 6 sums
LDS = {"k_plane_score": 256 * 4 * 8, "k_plane_chunks": 6 * 256 * 8}
# waves per SIMD: the score in 3-D keeps eight points' loads in flight in 72 registers -- one allocation step past 64, seven
# waves -- and is bound by LDS reads, not by occupancy (profiles/plane.md)
OCCUPANCY = {"k_plane_score": 7}


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_plane.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_plane_" in k}


def _kernel(name):
    return re.search(r"\d+(k_plane_[a-z_]+?)(?=I|E)", name).group(1)


def test_plane_kernels_spill_nothing_and_use_no_scratch_or_agprs():
    rep = _report()
    names = sorted(_kernel(k) for k in rep)
    assert names == sorted(k for k, n in INSTANCES.items() for _ in range(n)), names
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] <= LDS.get(_kernel(name), 0), name


def test_plane_kernels_keep_what_the_design_states():
    for name, r in _report().items():
        assert r["VGPRs"] <= BUDGET[_kernel(name)], (name, r["VGPRs"])
        assert r["Occupancy [waves/SIMD]"] >= OCCUPANCY.get(_kernel(name), 8), name
