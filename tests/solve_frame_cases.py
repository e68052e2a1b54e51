"""The table of solves of tests/test_gpu_solve_frame.py and the one function that runs a case, shared with the recorder at the
end of this file: the four CG drivers (cg_run, cg_run_poly, cg_run_poly_sr, cg_run_mg) on the paths where their host
scaffolding differs, each as assemble / solve / re-assemble the same points / solve again -- the second solve runs on what the
first one taught the context (predicted iteration counts, the unwatched coarse levels, the first look's burst).

    python tests/solve_frame_cases.py <commit> <out.json>      records the library FI_HIP_LIB names (default: the tree's)

driver: the function the finest level's solve runs in.  verify: set_verify_residual (None: the context's default).  env: test
switches of the library, set around the case.  ranks: a loop-back group of that many slabs.  zero_rhs: model rows and no
points.  timeout: FI_SOLVE_TIMEOUT_S=0, from a zero GUESS (no coarse-to-fine start in front of the driver under test)."""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np

from util import sphere_points

MG = dict(levels=2, multigrid=True)
MG_SIZES = [48, 40, 44]      # (tests/test_gpu_multilevel.py: three levels, the tail in the one-workgroup engine)


def _case(id, driver, sizes, dtype, n=600, **kw):
    return dict(id=id, driver=driver, sizes=sizes, dtype=dtype, n=n, **kw)


CASES = [
    _case("jacobi-3d-f32", "cg_run", [14, 12, 13], "f32", verify=False),
    _case("jacobi-3d-f64", "cg_run", [14, 12, 13], "f64", verify=False),
    _case("jacobi-3d-f32-verified", "cg_run", [14, 12, 13], "f32", verify=True),
    _case("jacobi-2d-f32", "cg_run", [40, 36], "f32", verify=False),
    _case("poly-3d-f32", "cg_run_poly", [14, 12, 13], "f32", poly=4),
    _case("poly-3d-f64", "cg_run_poly", [14, 12, 13], "f64", poly=4),
    _case("poly-2d-f32", "cg_run_poly", [40, 36], "f32", poly=4),
    _case("poly-odd-rows-f32", "cg_run_poly", [13, 11, 10], "f32", poly=4),
    _case("poly-slabs-f32", "cg_run_poly_sr", [16, 12, 24], "f32", poly=4, ranks=2),
    _case("poly-slabs-f64", "cg_run_poly_sr", [16, 12, 24], "f64", poly=4, ranks=2),
    _case("poly-slabs-two-reductions-f32", "cg_run_poly", [16, 12, 24], "f32", poly=4, ranks=2,
          env={"FI_NO_SINGLE_REDUCTION": "1"}),
    _case("poly-forced-single-reduction-f32", "cg_run_poly_sr", [14, 12, 13], "f32", poly=4,
          env={"FI_FORCE_SINGLE_REDUCTION": "1"}),
    _case("vcycle-f32", "cg_run_mg", MG_SIZES, "f32", n=2500, **MG),
    _case("vcycle-f64", "cg_run_mg", MG_SIZES, "f64", n=2500, **MG),
    _case("vcycle-mixed", "cg_run_mg", MG_SIZES, "f64", n=2500, mixed=True, **MG),
    _case("vcycle-f32-field-rule", "cg_run_mg", MG_SIZES, "f32", n=2500, field_tol=1e-5, **MG),
    _case("vcycle-slabs-mixed-kcycle", "cg_run_mg", MG_SIZES, "f64", n=2500, ranks=2, mixed=True, kcycle=1, coarse_tol=1e-2, **MG),
    _case("cascade-start-f32", "cg_run", MG_SIZES, "f32", n=2500, levels=2),
    _case("zero-rhs-jacobi", "cg_run", [14, 12, 13], "f32", zero_rhs=True),
    _case("zero-rhs-poly", "cg_run_poly", [14, 12, 13], "f32", poly=4, zero_rhs=True),
    _case("zero-rhs-poly-slabs", "cg_run_poly_sr", [16, 12, 24], "f32", poly=4, ranks=2, zero_rhs=True),
    _case("zero-rhs-vcycle", "cg_run_mg", MG_SIZES, "f32", zero_rhs=True, **MG),
    _case("timeout-jacobi", "cg_run", [14, 12, 13], "f32", timeout=True),
    _case("timeout-poly", "cg_run_poly", [14, 12, 13], "f32", poly=4, timeout=True),
    _case("timeout-poly-slabs", "cg_run_poly_sr", [16, 12, 24], "f32", poly=4, ranks=2, timeout=True),
    _case("timeout-vcycle", "cg_run_mg", MG_SIZES, "f32", n=2500, timeout=True, **MG),
]
IDS = [c["id"] for c in CASES]
BY_ID = {c["id"]: c for c in CASES}
DRIVERS = ("cg_run", "cg_run_poly", "cg_run_poly_sr", "cg_run_mg")

INT_FIELDS = ("iterations", "converged", "restarts", "field_rounds", "num_levels", "coarse_iterations", "operator_applies",
              "halo_exchanges", "reductions", "spmv_samples", "prec_samples")
HEX_FIELDS = ("rel_residual", "verified_residual", "field_estimate", "stop_residual")     # float.hex: every bit


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _build(fi, case, pts):
    if case.get("ranks"):
        f = fi.LatticeGroup(case["sizes"], case["ranks"], dtype=case["dtype"])
    else:
        f = fi.LatticeField(case["sizes"], dtype=case["dtype"])
    w = fi.Weights()
    f.add_field_constraints(w)
    if case.get("verify") is not None:
        for m in getattr(f, "members", [f]):
            m.set_verify_residual(case["verify"])
    if case.get("levels"):
        f.set_levels(case["levels"], case.get("coarse_tol"))
    if case.get("multigrid"):
        f.set_multigrid(True)
    if case.get("mixed"):
        f.set_mixed_precision(True)
    if case.get("kcycle"):
        f.set_kcycle(case["kcycle"])
    if case.get("field_tol"):
        f.set_field_tolerance(case["field_tol"])
    if case.get("poly"):
        f.set_polynomial(case["poly"])
    _add_points(fi, f, pts)
    return f


def _add_points(fi, f, pts):
    w = fi.Weights()
    if pts is not None:
        f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pts[0], pts[1], None)


def _solve(fi, f, case, guess):
    """one assemble + solve -> the recorded fields (FiError: its code and nothing else)"""
    tol = 1e-5 if case["dtype"] == "f32" else 1e-9
    try:
        f.assemble()
        res = f.solve_cg(guess, 3000, tol)
    except fi.FiError as e:
        if e.code == 2:     # FI_ERR_HIP: the device is in no state to go on with
            raise
        return {"error": e.code}
    if res is None:
        return {"error": 6}
    st = f.stats()
    out = {k: int(st[k]) for k in INT_FIELDS}
    out.update({k: float(st[k]).hex() for k in HEX_FIELDS})
    out["solution_sha256"] = hashlib.sha256(np.ascontiguousarray(f.solution_f64()).tobytes()).hexdigest()
    out["solution_is_zero"] = bool(not np.any(f.solution_f64()))
    return out


def run_case(fi, case):
    """-> [first solve, second solve] of the case, in a process state that remembers nothing of earlier contexts"""
    fi.memory_pool(0)
    rng = np.random.default_rng(sum(ord(ch) for ch in case["id"]))
    pts = None if case.get("zero_rhs") else sphere_points(rng, case["sizes"], case["n"])
    env = dict(case.get("env", {}))
    guess = None
    if case.get("timeout"):
        env["FI_SOLVE_TIMEOUT_S"] = "0"
        guess = np.zeros(int(np.prod(case["sizes"])), np.float32)
    with _environment(env):
        f = _build(fi, case, pts)
        first = _solve(fi, f, case, guess)
        for m in getattr(f, "members", [f]):     # the same points again: fi_assemble runs anew, the context keeps what it learnt
            m.clear_points()
        _add_points(fi, f, pts)
        second = _solve(fi, f, case, guess)
    return [first, second]


def record(fi, commit):
    return {"commit": commit, "cases": {case["id"]: run_case(fi, case) for case in CASES}}


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import field_interpolation_amd as fi
    with open(sys.argv[2], "w") as out:
        json.dump(record(fi, sys.argv[1]), out, indent=1, sort_keys=True)
        out.write("\n")
