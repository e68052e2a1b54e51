#!/usr/bin/env python3
"""Writes tests/golden/reference_rows.npz: rows, returns, error maps, upscaled fields and operator<< text recorded from the
REFERENCE's own compiled assembly (oracle/_ref/libfi_ref.so, built by build() where the reference's sources are at hand).
The keys are described in reference_rows.md.  tests/test_reference_rows.py imports this module: it holds the case
generator, the one function that drives a backend through a case, and the seeded cases of the live sweep.

usage (repository root, after build()):  python tests/golden/make_golden_reference.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F = np.float32
NPZ = os.path.join(HERE, "reference_rows.npz")

OP_VALUE, OP_VALUE_NEAREST, OP_GRADIENT = 0, 1, 2
WEIGHT_NAMES = ("data_pos", "data_gradient", "model_0", "model_1", "model_2", "model_3", "model_4", "gradient_smoothness")
KERNEL_PAIRS = [(vk, gk) for vk in (0, 1) for gk in (0, 1, 2)]
ALL_TERMS = dict(model_0=0.2, model_1=0.3, model_2=0.5, model_3=0.7, model_4=0.9, gradient_smoothness=0.4)
TERM_SETS = [dict(model_0=0.3), dict(model_1=0.7), dict(model_2=0.5), dict(model_3=0.9), dict(model_4=1.1),
             dict(gradient_smoothness=0.6), ALL_TERMS]
REGULAR = [[9], [7, 6], [5, 6, 4]]
NARROW = [[1], [2], [3], [4, 1], [2, 2], [1, 5, 2], [3, 2, 2]]
UPSCALES = [([5], [17]), ([4, 3], [9, 11]), ([3, 4, 2], [7, 5, 9]), ([2, 2], [2, 2]), ([5, 5], [3, 4]), ([1, 4], [5, 9]),
            ([4], [1])]


def _next(x, up):
    return np.nextafter(F(x), F(np.inf if up else -np.inf))


# One coordinate per edge the row builders can trip over, as a function of the axis length n.  No NaN, no infinity and
# nothing at or beyond 2^31: the reference casts those to int, which is undefined behaviour (reference_rows.md).
EDGE_COORDS = [
    lambda n: F(0), lambda n: F(1), lambda n: F(n - 1), lambda n: F(n), lambda n: F(-1),              # lattice hits
    lambda n: F(0.5), lambda n: F(1.5), lambda n: F(2.5), lambda n: F(n - 1.5),                       # k + 0.5:
    lambda n: F(-1.5), lambda n: F(-2.5),                                                             #   round != rint
    lambda n: F(-0.5), lambda n: _next(-0.5, True), lambda n: _next(-0.5, False),
    lambda n: _next(n - 1, True), lambda n: _next(n - 1, False),
    lambda n: F(n - 0.5), lambda n: _next(n - 0.5, True), lambda n: _next(n - 0.5, False),
    lambda n: F(-0.0), lambda n: F(1e6), lambda n: F(-1e6),
]
EDGE_WEIGHTS = [F(0), F(-0.75), F(1e-30)]


def make_case(name, sizes, weights, vk, gk, seed, npts=24, normals=True, point_weights=True, model_last=False):
    """One case: model rows, one add_points call, then single-constraint calls at every edge coordinate."""
    rng = np.random.default_rng(seed)
    D, n = len(sizes), int(np.prod(sizes))
    w = dict(data_pos=0.8, data_gradient=1.25, model_0=0.0, model_1=0.0, model_2=0.0, model_3=0.0, model_4=0.0,
             gradient_smoothness=0.0)
    w.update(weights)

    def other(d):
        if rng.random() < 0.5:
            return F(rng.uniform(0, sizes[d] - 1))
        return EDGE_COORDS[rng.integers(len(EDGE_COORDS))](sizes[d])

    edge = np.empty((len(EDGE_COORDS), D), F)
    for j, coord in enumerate(EDGE_COORDS):
        axis = (j + seed) % D
        for d in range(D):
            edge[j, d] = coord(sizes[d]) if d == axis else other(d)
    inner = np.stack([rng.uniform(-0.4, s - 0.6, 8) for s in sizes], 1).astype(F)
    pos = np.concatenate([edge[rng.permutation(len(edge))[:max(0, npts - 8)]], inner])
    pos = pos[rng.permutation(len(pos))]
    nrm = rng.normal(size=pos.shape).astype(F)
    nrm[::3, rng.integers(D)] = 0                                   # normals with a zero component
    pw = rng.uniform(0.2, 2.0, len(pos)).astype(F)
    pw[::5], pw[1::7], pw[2::9] = EDGE_WEIGHTS[0], EDGE_WEIGHTS[1], EDGE_WEIGHTS[2]

    m = 3 * len(edge)
    op_kind = np.tile(np.array([OP_VALUE, OP_VALUE_NEAREST, OP_GRADIENT], np.int32), len(edge))
    op_kernel = np.repeat((gk + np.arange(len(edge))) % 3, 3).astype(np.int32)     # every gradient kernel, in every case
    op_pos = np.repeat(edge, 3, axis=0)
    op_grad = rng.normal(size=(m, D)).astype(F)
    op_grad[::4, rng.integers(D)] = 0
    op_value = rng.normal(size=m).astype(F)                                         # per-point value targets
    op_weight = rng.uniform(0.3, 1.5, m).astype(F)
    for k, ew in enumerate(EDGE_WEIGHTS):
        op_weight[7 + k::11] = ew
    return dict(name=name, sizes=np.asarray(sizes, np.int32), weights=np.array([w[k] for k in WEIGHT_NAMES], F),
                kernels=np.array([vk, gk], np.int32), flags=np.array([int(model_last), 0], np.int32),
                pos=pos, nrm=nrm if normals else np.empty((0, D), F), pw=pw if point_weights else np.empty(0, F),
                op_kind=op_kind, op_kernel=op_kernel, op_pos=op_pos, op_grad=op_grad, op_value=op_value, op_weight=op_weight,
                x=rng.normal(size=n).astype(F))


def readme_case():
    """The worked example of the reference's README (six unknowns, eight rows), through the public calls."""
    c = make_case("readme", [6], dict(data_pos=1.0, data_gradient=1.0, model_2=1.0), 1, 0, 0, model_last=True)
    c["flags"] = np.array([1, 1], np.int32)                         # model rows last; record operator<<
    c["pos"], c["nrm"], c["pw"] = np.empty((0, 1), F), np.empty((0, 1), F), np.empty(0, F)
    c["op_kind"] = np.array([OP_VALUE, OP_VALUE, OP_GRADIENT, OP_GRADIENT], np.int32)
    c["op_kernel"] = np.zeros(4, np.int32)
    c["op_pos"] = np.array([[0], [5], [0], [4]], F)
    c["op_grad"] = np.array([[0], [0], [1], [-1]], F)
    c["op_value"] = np.array([4, 2, 0, 0], F)
    c["op_weight"] = np.ones(4, F)
    return c


def fixture_cases():
    cases, seed = [readme_case()], 100
    for sizes in REGULAR:
        tag = "%dd" % len(sizes)
        for vk, gk in KERNEL_PAIRS:                                 # every value x gradient kernel pair
            seed += 1
            cases.append(make_case("%s_kernels_v%dg%d" % (tag, vk, gk), sizes, dict(model_2=0.5), vk, gk, seed))
        for k, terms in enumerate(TERM_SETS):                       # each model term alone, then all together
            seed += 1
            vk, gk = KERNEL_PAIRS[(k + len(sizes)) % 6]
            label = "all" if terms is ALL_TERMS else next(iter(terms))
            cases.append(make_case("%s_%s" % (tag, label), sizes, terms, vk, gk, seed, npts=16))
    for k, sizes in enumerate(NARROW):                              # lattices narrower than the stencils
        seed += 1
        vk, gk = KERNEL_PAIRS[k % 6]
        cases.append(make_case("narrow_" + "x".join(map(str, sizes)), sizes, ALL_TERMS, vk, gk, seed, npts=16))
    seed += 1                                                       # the optional arrays left out: no normals, no weights
    cases.append(make_case("2d_values_only", [7, 6], dict(model_2=0.5), 1, 1, seed, normals=False, point_weights=False))
    cases.append(make_case("3d_unweighted", [5, 6, 4], dict(model_1=0.4), 0, 2, seed + 1, npts=16, point_weights=False))
    return cases


def sweep_case(seed):
    """A fresh case of the live sweep: the same axes, drawn at random."""
    rng = np.random.default_rng(50_000 + seed)
    pool = REGULAR + NARROW + [[12], [4, 9], [6, 2, 5], [3, 3, 3]]
    sizes = pool[rng.integers(len(pool))]
    terms = {k: F(rng.uniform(0.05, 2.0)) for k in ALL_TERMS if rng.random() < 0.5}
    terms.update(data_pos=F(rng.uniform(0.1, 3.0)), data_gradient=F(rng.uniform(0.1, 3.0)))
    vk, gk = KERNEL_PAIRS[rng.integers(6)]
    return make_case("sweep%d" % seed, sizes, terms, vk, gk, 1000 + seed, npts=int(rng.integers(8, 30)),
                     point_weights=bool(rng.random() < 0.8), model_last=bool(rng.random() < 0.3))


def run_case(backend, case):
    """Drives `backend` (oracle.fi_ref, oracle.fi_oracle: the same method names) through a case; returns what is recorded."""
    w = backend.Weights(value_kernel=int(case["kernels"][0]), gradient_kernel=int(case["kernels"][1]),
                        **{k: float(v) for k, v in zip(WEIGHT_NAMES, case["weights"])})
    f = backend.LatticeField([int(s) for s in case["sizes"]])
    model_last = bool(case["flags"][0])
    if not model_last:
        f.add_field_constraints(w)
    if len(case["pos"]):
        f.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, case["pos"],
                     case["nrm"] if len(case["nrm"]) else None, case["pw"] if len(case["pw"]) else None)
    returns = np.zeros(len(case["op_kind"]), np.uint8)
    for k, kind in enumerate(case["op_kind"]):
        p, g = case["op_pos"][k], case["op_grad"][k]
        v, cw = float(case["op_value"][k]), float(case["op_weight"][k])
        if kind == OP_VALUE:
            returns[k] = f.add_value_constraint(p, v, cw)
        elif kind == OP_VALUE_NEAREST:
            returns[k] = f.add_value_constraint_nearest_neighbor(p, g, v, cw)
        else:
            returns[k] = f.add_gradient_constraint(p, g, cw, int(case["op_kernel"][k]))
    if model_last:
        f.add_field_constraints(w)
    rows, cols, vals, rhs = f.get()
    out = dict(rows=rows, cols=cols, vals=vals.view(np.uint32), rhs=rhs.view(np.uint32),
               counts=np.array([f.num_rows, f.num_triplets], np.int64), returns=returns,
               errmap=f.error_map(case["x"]).view(np.uint32))
    if case["flags"][1] and hasattr(f, "text"):
        out["text"] = np.frombuffer(f.text(), np.uint8)
    return out


INPUT_KEYS = ("sizes", "weights", "kernels", "flags", "pos", "nrm", "pw", "op_kind", "op_kernel", "op_pos", "op_grad",
              "op_value", "op_weight", "x")
OUTPUT_KEYS = ("rows", "cols", "vals", "rhs", "counts", "returns", "errmap")


def upscale_inputs():
    rng = np.random.default_rng(77)
    return [(np.asarray(s, np.int32), np.asarray(l, np.int32), rng.normal(size=int(np.prod(s))).astype(F))
            for s, l in UPSCALES]


PER_AXIS = ("pos", "nrm", "op_pos", "op_grad")                   # stored flat; (-1, D) again in load()


def generate(backend):
    """Every array of the fixture, made with `backend`.  The arrays of all cases are stored end to end under one key each,
    with `<key>_start` giving where every case begins (one entry more than there are cases)."""
    cases = fixture_cases()
    done = []
    for c in cases:
        r = dict(c)
        r.update(run_case(backend, c))
        done.append(r)
    out = {"names": np.array([c["name"] for c in cases])}
    for k in INPUT_KEYS + OUTPUT_KEYS + ("text",):
        parts = [np.ravel(r[k]) if k in r else np.empty(0, np.uint8) for r in done]
        out[k] = np.concatenate(parts)
        out[k + "_start"] = np.cumsum([0] + [p.size for p in parts]).astype(np.int64)
    for j, (small, large, field) in enumerate(upscale_inputs()):
        out["u%d_small_sizes" % j], out["u%d_large_sizes" % j], out["u%d_field" % j] = small, large, field
        out["u%d_out" % j] = backend.upscale_field(field, small, large).view(np.uint32)
    return out


def load(path=NPZ):
    """The fixture as (cases, upscales): each case a dict of its inputs and recorded outputs."""
    z = np.load(path)
    cases = []
    for i, name in enumerate(z["names"]):
        c = {"name": str(name)}
        for k in INPUT_KEYS + OUTPUT_KEYS + ("text",):
            start = z[k + "_start"]
            c[k] = z[k][start[i]:start[i + 1]]
        D = len(c["sizes"])
        for k in PER_AXIS:
            c[k] = c[k].reshape(-1, D)
        cases.append(c)
    ups = [{k: z["u%d_%s" % (j, k)] for k in ("small_sizes", "large_sizes", "field", "out")} for j in range(len(UPSCALES))]
    return cases, ups


def main():
    from oracle import fi_ref
    if not fi_ref.available():
        sys.exit("oracle/_ref/libfi_ref.so is missing: run build() with the reference's sources at hand")
    out = generate(fi_ref)
    np.savez_compressed(NPZ, **out)
    print("wrote %s: %d cases, %d upscales, %d bytes" % (os.path.relpath(NPZ, ROOT), len(out["names"]), len(UPSCALES),
                                                         os.path.getsize(NPZ)))


if __name__ == "__main__":
    main()
