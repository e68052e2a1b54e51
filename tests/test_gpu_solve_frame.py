"""The four CG drivers against what the commit before the shared solve frame computed: tests/golden/solve_frame_parent.json
holds, for every case of tests/solve_frame_cases.py, the integers of fi_stats, its residual figures bit for bit and the
SHA-256 of the fp64 solution, recorded twice with that commit's library (the two recordings agreed in every field; the
fixture names the commit).  The frame (fi_solver_internal.h, SolveFrame) and the Chebyshev recurrence (fi_cheb.h) are host
code that must not move a launch or a constant, so the working tree has to give the same fields, every one.

A compiler or ROCm change that moves bits makes this test fail without any fault of the drivers: record the fixture anew
from the then-parent commit (python tests/solve_frame_cases.py <commit> <file>, with FI_HIP_LIB naming that commit's
library) -- and look at the INTEGER mismatches first: an iteration count, a restart or a sample count that differs says
which path changed; the hexadecimal figures and the hash only say that something did."""
import json
import os

import pytest

import solve_frame_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_frame_parent.json")


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_covers_every_driver(golden):
    """every driver keeps at least two cases with a solution hash, one in each precision"""
    assert sorted(golden["cases"]) == sorted(cases.IDS) and golden["commit"]
    for driver in cases.DRIVERS:
        hashed = {c["dtype"] for c in cases.CASES if c["driver"] == driver and "solution_sha256" in golden["cases"][c["id"]][0]
                  and not c.get("zero_rhs")}
        assert hashed == {"f32", "f64"}, (driver, hashed)


@pytest.mark.parametrize("case_id", cases.IDS)
def test_solves_match_the_parent_commit(fi, golden, case_id):
    case = cases.BY_ID[case_id]
    want = golden["cases"][case_id]
    got = cases.run_case(fi, case)
    assert len(got) == len(want) == 2
    for k, (g, w) in enumerate(zip(got, want)):
        wrong = sorted(name for name in set(g) | set(w) if g.get(name) != w.get(name))
        wrong.sort(key=lambda name: name not in cases.INT_FIELDS)      # the integers first
        assert not wrong, (case_id, "solve %d" % (k + 1), [(name, g.get(name), w.get(name)) for name in wrong])
    if case.get("timeout"):
        assert [s.get("error") for s in got] == [7, 7]                # FI_ERR_TIMEOUT, at the first guard
    if case.get("zero_rhs"):
        for s in got:                                                    # done == 4: x = 0, converged
            assert s["solution_is_zero"] and s["converged"] == 1 and s["iterations"] == 0
