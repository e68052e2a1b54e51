"""The clustering kernels (fi_cluster.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_cluster.usage.txt): every kernel instance is there, none has VGPR or SGPR spills, scratch or
AGPRs, the three walking kernels use no LDS and hold 8 waves per SIMD -- the walk they extend, k_cloud_radius, holds 8 at 32
VGPRs, and a core byte and two roots do not cost 32 more -- and registers stay within DESIGN.md 4.20's table."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")

# DESIGN.md 4.20's table: what hipcc reports for gfx950, rounded up to the next multiple of 8 (the largest instance where a
# kernel is a template over the dimension)
BUDGET = {"k_cluster_start": 8, "k_cluster_core": 32, "k_cluster_join": 32, "k_cluster_jump": 8, "k_cluster_roots": 8,
          "k_cluster_border": 32, "k_cluster_keys": 8, "k_cluster_first": 16, "k_cluster_chunk_counts": 8, "k_cluster_chunks": 24,
          "k_cluster_rows": 48}
# how many instances of each the unit holds: the walks and the chunk sums over D
INSTANCES = {"k_cluster_start": 1, "k_cluster_core": 3, "k_cluster_join": 3, "k_cluster_jump": 1, "k_cluster_roots": 1,
             "k_cluster_border": 3, "k_cluster_keys": 1, "k_cluster_first": 1, "k_cluster_chunk_counts": 1, "k_cluster_chunks": 3,
             "k_cluster_rows": 1}
WALKS = ("k_cluster_core", "k_cluster_join", "k_cluster_border")
# bytes a block of the chunk sums in 3-D: per axis 256 doubles and twice 256 floats, and 256 counts
LDS = {"k_cluster_chunks": 3 * 256 * (8 + 4 + 4) + 256 * 4}


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_cluster.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_cluster_" in k}


def _kernel(name):
    return re.search(r"\d+(k_cluster_[a-z_]+?)(?=I|E)", name).group(1)


def test_cluster_kernels_spill_nothing_and_use_no_scratch_or_agprs():
    rep = _report()
    names = sorted(_kernel(k) for k in rep)
    assert names == sorted(k for k, n in INSTANCES.items() for _ in range(n)), names
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] <= LDS.get(_kernel(name), 0), name


def test_the_walking_kernels_use_no_lds_and_hold_eight_waves():
    walks = {name: r for name, r in _report().items() if _kernel(name) in WALKS}
    assert len(walks) == 9
    for name, r in walks.items():
        assert r["LDS Size [bytes/block]"] == 0, name
        assert r["Occupancy [waves/SIMD]"] >= 8, (name, r["Occupancy [waves/SIMD]"])
        assert r["VGPRs"] <= 64, (name, r["VGPRs"])            # 512 registers a lane over 8 waves


def test_cluster_kernels_keep_what_the_design_states():
    for name, r in _report().items():
        assert r["VGPRs"] <= BUDGET[_kernel(name)], (name, r["VGPRs"])
        assert r["Occupancy [waves/SIMD]"] >= 8, name
