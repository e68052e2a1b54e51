"""The point-cloud kernels (fi_cloud.hip) against the compiler's resource report the build keeps next to the object
(field_interpolation_amd/csrc/fi_cloud.usage.txt): every kernel instance is there, none has VGPR or SGPR spills, scratch or
AGPRs, the two walking kernels use no LDS, and registers stay within DESIGN.md 4.19's table.  The occupancy floors are the
project's own: the neighbour walk keeps k_knn_query's 8 / 8 / 5 waves per SIMD at the capacities 8 / 16 / 32
-- leaving the point itself out by its index is what keeps k = 16 in the class of 16 -- and the radius walk, which holds no
list, keeps k_nearest_query's 8."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "field_interpolation_amd", "csrc")

# DESIGN.md 4.19's table: what hipcc reports for gfx950, rounded up to the next multiple of 8 (the largest instance where a
# kernel is a template over the dimension; the neighbour walk by capacity)
BUDGET = {"k_cloud_radius": 32, "k_cloud_neighbours": {8: 48, 16: 64, 32: 96}, "k_cloud_blank": 8, "k_cloud_block_sums": 16,
          "k_cloud_finish": 16, "k_cloud_keep": 8, "k_cloud_thin_keys": 24, "k_cloud_thin_heads": 8, "k_cloud_thin_assign": 8,
          "k_cloud_thin_cells": 40}
# how many instances of each the unit holds: the radius walk over D and over whose points the queries are, the neighbour
# walk over D and the capacity, the sums over their two passes, the thinning over D
INSTANCES = {"k_cloud_radius": 6, "k_cloud_neighbours": 9, "k_cloud_blank": 1, "k_cloud_block_sums": 2, "k_cloud_finish": 2,
             "k_cloud_keep": 1, "k_cloud_thin_keys": 3, "k_cloud_thin_heads": 1, "k_cloud_thin_assign": 1, "k_cloud_thin_cells": 3}
# bytes a block: 256 doubles and 256 counts of the tree sum
LDS = {"k_cloud_block_sums": 256 * 8 + 256 * 4}
OCCUPANCY = {8: 8, 16: 8, 32: 5}


def _report():
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "fi_cloud.usage.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_cloud_" in k}


def _kernel(name):
    return re.search(r"\d+(k_cloud_[a-z_]+?)(?=I|E)", name).group(1)


def _capacity(name):
    """the template arguments (D, CAP) of a mangled k_cloud_neighbours"""
    m = re.search(r"k_cloud_neighboursILi(\d+)ELi(\d+)E", name)
    return int(m.group(1)), int(m.group(2))


def test_cloud_kernels_spill_nothing_and_use_no_scratch_or_agprs():
    rep = _report()
    names = sorted(_kernel(k) for k in rep)
    assert names == sorted(k for k, n in INSTANCES.items() for _ in range(n)), names
    assert sorted(_capacity(k) for k in rep if "k_cloud_neighbours" in k) == [(d, c) for d in (1, 2, 3) for c in (8, 16, 32)]
    for name, r in rep.items():
        assert r["VGPRs Spill"] == 0, name
        assert r["SGPRs Spill"] == 0, name
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["AGPRs"] == 0, name
        assert r["LDS Size [bytes/block]"] <= LDS.get(_kernel(name), 0), name


def test_the_walking_kernels_use_no_lds_and_keep_their_waves():
    for name, r in _report().items():
        if _kernel(name) == "k_cloud_radius":
            assert r["LDS Size [bytes/block]"] == 0 and r["Occupancy [waves/SIMD]"] >= 8, (name, r)
        elif _kernel(name) == "k_cloud_neighbours":
            assert r["LDS Size [bytes/block]"] == 0, name
            assert r["Occupancy [waves/SIMD]"] >= OCCUPANCY[_capacity(name)[1]], (name, r["Occupancy [waves/SIMD]"])


def test_cloud_kernels_keep_what_the_design_states():
    for name, r in _report().items():
        budget = BUDGET[_kernel(name)]
        if isinstance(budget, dict):
            budget = budget[_capacity(name)[1]]
        assert r["VGPRs"] <= budget, (name, r["VGPRs"])
        if _kernel(name) not in ("k_cloud_radius", "k_cloud_neighbours"):
            assert r["Occupancy [waves/SIMD]"] >= 8, name
