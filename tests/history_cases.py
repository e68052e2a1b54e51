"""The table of solver cases of tests/test_gpu_history.py and the builders both of its arms share: the same call sequence
makes the clean answer and the answer after a polluted history, so that only the history differs between the two."""
import numpy as np

from util import sphere_points

# path: what the case is there for.  data: "values" (value rows, no gradient rows: Weights(data_gradient=0)) or "oriented"
# (points with normals, default weights).  tol / max_it: the solve's; a capped solve is compared as it stands -- an iterate
# is as good a witness of a stale read as a converged field.  extras: jacobi, tile_pass and error_map follow the solve.
# converges: a remembered bound or prediction lies on the case's path and the solve ends by its stop rule well below max_it:
# the cases of arm D (tests/test_gpu_history.py says there why 1, 2, 3, 10 and 11 are not among them).
# tail: named for a level in the one-workgroup engine; checked against FI_NO_TAIL.
# Case 12 runs on 29 x 31 x 40, not the 24 x 20 x 40 first named for it: a level needs 8 points per axis (plan_levels), and
# 24 x 20 x 40 stops at one coarse level.  29 x 31 x 40 gives 15 x 16 x 20 in slabs and 8 x 8 x 10 as the replicated tail.
CASES = [
    dict(id="1-line-f32", path="Jacobi-PCG, 1-D generic kernel", sizes=[97], dtype="f32", data="values", n=40,
         tol=1e-5, max_it=400, extras=True),
    dict(id="1-line-f64", path="Jacobi-PCG, 1-D generic kernel", sizes=[97], dtype="f64", data="values", n=40,
         tol=1e-8, max_it=400, extras=True),
    dict(id="2-tile2d-f32", path="Jacobi-PCG, 2-D tile kernel, rows of 131", sizes=[131, 67], dtype="f32", data="values", n=900,
         tol=1e-5, max_it=400, extras=True),
    dict(id="2-tile2d-f64", path="Jacobi-PCG, 2-D tile kernel, rows of 131", sizes=[131, 67], dtype="f64", data="values", n=900,
         tol=1e-8, max_it=400, extras=True),
    dict(id="3-march-f32", path="Jacobi-PCG, 3-D marching kernel, odd extents", sizes=[41, 37, 33], dtype="f32", data="values",
         n=5000, tol=1e-5, max_it=400, extras=True),
    dict(id="3-march-f64", path="Jacobi-PCG, 3-D marching kernel, odd extents", sizes=[41, 37, 33], dtype="f64", data="values",
         n=5000, tol=1e-8, max_it=400, extras=True),
    dict(id="4-poly-f32", path="polynomial PCG, 4 terms", sizes=[41, 37, 33], dtype="f32", data="values", n=5000,
         tol=1e-5, max_it=400, poly=4, converges=True),
    dict(id="5-start-cubic-f64", path="coarse-to-fine start, cubic", sizes=[41, 37, 33], dtype="f64", data="values", n=5000,
         tol=1e-8, max_it=4000, levels=2, coarse_tol=1e-4, num_levels=3, converges=True),
    dict(id="5-start-linear-f64", path="coarse-to-fine start, FI_LINEAR_START", sizes=[41, 37, 33], dtype="f64", data="values",
         n=5000, tol=1e-8, max_it=4000, levels=2, coarse_tol=1e-4, num_levels=3, env={"FI_LINEAR_START": "1"}, converges=True),
    dict(id="6-vcycle-poly-f32", path="V-cycle PCG, polynomial smoother; 21.19.17 tiled, 11.10.9 in one workgroup",
         sizes=[41, 37, 33], dtype="f32", data="values", n=5000, tol=1e-5, max_it=200, levels=2, coarse_tol=1e-4, num_levels=3,
         multigrid=True, converges=True, tail=True),
    dict(id="7-vcycle-mixed-field-rule", path="V-cycle, fp64 CG + fp32 replica, field stop rule", sizes=[48, 40, 36], dtype="f64",
         data="values", n=5000, tol=1e-8, max_it=200, levels=2, coarse_tol=1e-4, num_levels=3, multigrid=True, mixed=True,
         field_tol=1e-5, converges=True),
    dict(id="8-vcycle-cheb-2d-f64", path="V-cycle, Chebyshev smoother in the full operator, oriented points", sizes=[131, 67],
         dtype="f64", data="oriented", n=900, tol=1e-8, max_it=400, levels=3, coarse_tol=1e-4, num_levels=4, multigrid=True,
         converges=True),
    dict(id="9-kcycle-mixed", path="K-cycle on the first coarse level, fp64 CG + fp32 replica", sizes=[48, 40, 36], dtype="f64",
         data="values", n=5000, tol=1e-8, max_it=200, levels=2, coarse_tol=1e-4, num_levels=3, multigrid=True, mixed=True,
         kcycle=1, converges=True),
    dict(id="10-wide-rows-f32", path="wide rows: model_3, gradient_smoothness", sizes=[37, 41, 30], dtype="f32", data="values",
         n=5000, tol=1e-5, max_it=300, weights=dict(model_2=0.3, model_3=0.7, gradient_smoothness=0.3)),
    dict(id="11-triplets-f64", path="triplet rows (add_rows_coo): 300 rows on 2 000 unknowns, tile_pass", sizes=[50, 40],
         dtype="f64", data="values", n=300, tol=1e-8, max_it=400, coo=300, tile=True),
    dict(id="12-slabs-vcycle-f32", path="3 slabs, V-cycle, levels 2", sizes=[29, 31, 40], dtype="f32", data="values", n=3000,
         tol=1e-5, max_it=200, levels=2, coarse_tol=1e-4, num_levels=3, multigrid=True, ranks=3, converges=True),
    dict(id="12-slabs-vcycle-mixed", path="3 slabs, V-cycle, fp64 CG + fp32 replica, levels 2", sizes=[29, 31, 40], dtype="f64",
         data="values", n=3000, tol=1e-8, max_it=200, levels=2, coarse_tol=1e-4, num_levels=3, multigrid=True, mixed=True,
         ranks=3, converges=True),
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]
SHRINK_IDS = [c["id"] for c in CASES if len(c["sizes"]) == 3 and not c.get("ranks")]      # (the issue's: value rows, 3-D)
CACHE_IDS = [c["id"] for c in CASES if c.get("converges")]                                  # arm D
TAIL_IDS = [c["id"] for c in CASES if c.get("tail")]


def seed_of(case, salt=0):
    return sum(ord(ch) for ch in case["id"]) * 7 + salt


def points(case, salt=0, n=None, data=None):
    """-> (positions, normals or None, values or None) inside the case's own lattice, whatever lattice they go to"""
    sizes = case["sizes"]
    rng = np.random.default_rng(seed_of(case, salt))
    n = case["n"] if n is None else n
    data = case["data"] if data is None else data
    if data == "oriented":
        if len(sizes) == 1:
            pos = rng.uniform(0.0, sizes[0] - 1.0, (n, 1)).astype(np.float32)
            return pos, np.where(rng.random((n, 1)) < 0.5, -1.0, 1.0).astype(np.float32), None
        pos, nrm = sphere_points(rng, sizes, n, noise=0.4)
        return pos, nrm, None
    pos = np.stack([rng.uniform(0.0, s - 1.0, n) for s in sizes], axis=1).astype(np.float32)
    return pos, None, rng.normal(size=n).astype(np.float32)


def triplets(case, salt=0):
    """case["coo"] rows of three entries each over the lattice's unknowns (a repeated column now and then: summed)"""
    rng = np.random.default_rng(seed_of(case, 1000 + salt))
    m, n = case["coo"], int(np.prod(case["sizes"]))
    rows = np.repeat(np.arange(m), 3)
    cols = rng.integers(0, n, 3 * m)
    cols[1::30] = cols[0::30]                       # every tenth row names a column twice
    vals = rng.normal(size=3 * m).astype(np.float32)
    return rows, cols, vals, rng.normal(size=m).astype(np.float32)


def weights(fi, case):
    kw = dict(case.get("weights", {}))
    if case["data"] == "values":
        kw["data_gradient"] = 0.0
    return fi.Weights(**kw)


def add_data(fi, f, case, w, pts):
    pos, nrm, val = pts
    f.add_points(w.data_pos, w.value_kernel, 1.0 if nrm is not None else 0.0, w.gradient_kernel, pos, nrm, None, values=val)


def make(fi, case, pts, sizes=None, coo_salt=0):
    """A context (or loop-back group) of the case's solver path over `sizes` (default: the case's) holding `pts`, not
    yet assembled"""
    sizes = case["sizes"] if sizes is None else sizes
    if case.get("ranks"):
        f = fi.LatticeGroup(sizes, case["ranks"], dtype=case["dtype"])
    else:
        f = fi.LatticeField(sizes, dtype=case["dtype"])
    w = weights(fi, case)
    f.add_field_constraints(w)
    if case.get("levels"):
        f.set_levels(case["levels"], case["coarse_tol"])
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
    add_data(fi, f, case, w, pts)
    if case.get("coo"):      # (columns of the case's own lattice: in range of a larger one too)
        f.add_rows_coo(*triplets(case, coo_salt))
    return f


def num_unknowns(f):
    return int(np.prod(f.sizes))


def probe(case, n=None):
    """the fixed input of the calls that follow the solve (jacobi, tile_pass, error_map): one value per unknown of the
    lattice it goes to (default: the case's own)"""
    n = int(np.prod(case["sizes"])) if n is None else n
    return np.random.default_rng(seed_of(case, 77)).normal(size=n).astype(np.float32)


def answer(f, case):
    """Assemble, solve from the context's own start, and read everything back -> dict of arrays and numbers.  The same calls
    in the same order for every history."""
    f.assemble()
    res = f.solve_cg(None, case["max_it"], case["tol"])
    assert res is not None, "breakdown"
    x, it, rel = res
    st = f.stats()
    out = {"x": np.array(x, copy=True), "iterations": it, "relative_residual": np.float32(rel), "solution_f64": f.solution_f64(),
           "true_residual": f.true_residual(), "coarse_iterations": st["coarse_iterations"], "converged": st["converged"],
           "num_levels": st["num_levels"], "field_rounds": st["field_rounds"], "field_estimate": st["field_estimate"]}
    if case.get("extras") or case.get("tile"):
        g = probe(case, num_unknowns(f))
        out["tile_pass"] = np.array(f.tile_pass(g, 8), copy=True)
    if case.get("extras"):
        out["jacobi"] = np.array(f.jacobi(g, 3, 0.7), copy=True)
        out["error_map"] = np.array(f.error_map(g), copy=True)
    return out


def poison(f, case, FiError):
    """NaN into every floating vector a bounded call reaches.  The solves end whatever the numbers do: a non-finite r.r or
    p.Ap raises the stop flag in the step that meets it (cg_logic, k_cg_xp_f, k_pcg_*, k_mg_logic: done = 2, or 1 then 5 at
    the V-cycle's first residual), widenings of a polynomial's interval need finite sums, restarts are counted down from 3,
    and max_iterations = 2 ends what is left.  A second solve from a finite guess of size 1e15 runs two whole iterations, so
    that the preconditioner's vectors -- every level's, the replica's -- hold that history too."""
    n = num_unknowns(f)
    nan32, nan64 = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float64)
    big = (np.random.default_rng(n).choice([-1.0, 1.0], n) * 1e15).astype(np.float32)

    def solve(guess):
        try:
            f.solve_cg(guess, 2, case["tol"])
        except FiError as e:
            if e.code != 6:     # FI_ERR_BREAKDOWN is what NaN is expected to end in
                raise

    solve(big)
    f.apply_AtA(nan64)
    if hasattr(f, "jacobi"):
        f.jacobi(nan32, 1, 1.0)
    f.error_map(nan32)
    solve(nan32)
