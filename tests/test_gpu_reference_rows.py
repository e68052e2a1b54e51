"""The device library against the reference's OWN compiled assembly, as recorded in tests/golden/reference_rows.npz
(tests/golden/reference_rows.md; CPU side: tests/test_reference_rows.py).  Nothing here calls the oracle: the float64 normal
equations are formed with scipy from the reference's recorded triplets, the returns, upscaled fields and error maps are the
reference's recorded ones.  Tolerances are the project's existing ones: operator pieces 1e-12 (fp64 contexts) and 2e-6 (fp32)
as in test_gpu_operator._check_operator, whose two x vectors are used; error map 2e-4 of the largest entry as in
test_gpu_solve.test_error_map_equals_reference_blame (the reference sums it in fp32); upscale: equal bits."""
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import reference_rows as rr
from reference_rows import golden
from test_gpu_operator import _check_operator

pytestmark = pytest.mark.gpu

CASES, UPSCALES = rr.fixture()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1, "no HIP device visible"
    return fi


class _RecordedSystem:
    """The reference's recorded rows of a case behind the two members _check_operator reads."""

    def __init__(self, case):
        self.num_unknowns = int(np.prod(case["sizes"]))
        vals = case["vals"].view(np.float32).astype(np.float64)
        A = sp.coo_matrix((vals, (case["rows"], case["cols"])), shape=(int(case["counts"][0]), self.num_unknowns)).tocsr()
        self._AtA = (A.T @ A).tocsc()
        self._atb = A.T @ case["rhs"].view(np.float32).astype(np.float64)

    def normal_equations(self):
        return self._AtA, self._atb, self._AtA.diagonal()


def _replay(fi, case, dtype):
    """The case's call sequence on the device library -> (field, returns of the single-constraint calls)."""
    w = fi.Weights(value_kernel=fi.ValueKernel(int(case["kernels"][0])), gradient_kernel=fi.GradientKernel(int(case["kernels"][1])),
                   **{k: float(v) for k, v in zip(golden.WEIGHT_NAMES, case["weights"])})
    fg = fi.LatticeField([int(s) for s in case["sizes"]], dtype=dtype)
    fg.add_field_constraints(w)                    # the model is kept apart from the rows: its place in the order is moot
    if len(case["pos"]):
        fg.add_points(float(case["weights"][0]), w.value_kernel, float(case["weights"][1]), w.gradient_kernel, case["pos"],
                      case["nrm"] if len(case["nrm"]) else None, case["pw"] if len(case["pw"]) else None)
    returns = np.zeros(len(case["op_kind"]), np.uint8)
    for k, kind in enumerate(case["op_kind"]):
        p, g = case["op_pos"][k], case["op_grad"][k]
        v, cw = float(case["op_value"][k]), float(case["op_weight"][k])
        if kind == golden.OP_VALUE:
            returns[k] = fg.add_value_constraint(p, v, cw)
        elif kind == golden.OP_VALUE_NEAREST:
            returns[k] = fg.add_value_constraint_nearest_neighbor(p, g, v, cw)
        else:
            returns[k] = fg.add_gradient_constraint(p, g, cw, int(case["op_kernel"][k]))
    return fg, returns


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_operator_pieces_equal_the_reference_rows(fi, case, dtype):
    """Atb(), diag() and apply_AtA(x) against the float64 normal equations of the reference's own triplets: edge positions,
    zero / negative / 1e-30 weights, value targets, every kernel and model term, lattices narrower than the stencils."""
    fg, _ = _replay(fi, case, dtype)
    _check_operator(_RecordedSystem(case), fg, dtype)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_single_constraint_returns_equal_the_reference(fi, case):
    _, returns = _replay(fi, case, "f32")
    bad = np.flatnonzero(returns != case["returns"])
    assert bad.size == 0, "call %s: kind %s kernel %s at %s weight %s: got %s, the reference returned %s" % (
        bad[:4], case["op_kind"][bad[:4]], case["op_kernel"][bad[:4]], case["op_pos"][bad[:4]].tolist(),
        case["op_weight"][bad[:4]], returns[bad[:4]], case["returns"][bad[:4]])


def test_upscale_field_equals_the_reference_bits(fi):
    for u in UPSCALES:
        got = fi.upscale_field(u["field"], [int(s) for s in u["small_sizes"]], [int(s) for s in u["large_sizes"]])
        assert got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), u["out"]), (u["small_sizes"], u["large_sizes"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_error_map_equals_the_reference(fi, case, dtype):
    fg, _ = _replay(fi, case, dtype)
    expect = case["errmap"].view(np.float32)
    heat = fi.generate_error_map(fg, case["x"])
    assert heat.dtype == np.float32 and heat.shape == expect.shape
    assert np.abs(heat - expect).max() <= 2e-4 * np.abs(expect).max()


def test_dropin_device_calls_equal_the_reference(tmp_path):
    """The C++ drop-in's generate_error_map (on the rows its host builders made) and upscale_field, through dump_rows --device;
    GpuLatticeField's single-constraint calls return what the reference returned."""
    cases_file, out = str(tmp_path / "cases.txt"), str(tmp_path / "device.txt")
    rr.write_case_file(cases_file, CASES, UPSCALES)
    run = subprocess.run([rr.build_dropin_exe(), "--device", cases_file, out], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    maps, ups, rets = rr.parse_device_dump(open(out).read())
    assert len(maps) == len(CASES) and len(ups) == len(UPSCALES) and len(rets) == len(CASES)
    for c, got in zip(CASES, rets):
        assert np.array_equal(got, c["returns"]), (c["name"], np.flatnonzero(got != c["returns"])[:5])
    for c, bits in zip(CASES, maps):
        expect = c["errmap"].view(np.float32)
        assert bits.shape == expect.shape, c["name"]
        assert np.abs(bits.view(np.float32) - expect).max() <= 2e-4 * np.abs(expect).max(), c["name"]
    for u, bits in zip(UPSCALES, ups):
        assert np.array_equal(bits, u["out"]), (u["small_sizes"], u["large_sizes"])
