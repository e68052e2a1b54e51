"""The oracle and the drop-in's host row builders, held to the reference's OWN compiled assembly.

tests/golden/reference_rows.npz was recorded from oracle/_ref/libfi_ref.so -- the reference's field_interpolation.cpp as it
stands plus add_equation / operator<< from the head of its sparse_linear.cpp (oracle/Makefile) -- by
tests/golden/make_golden_reference.py.  Three legs:
  * the oracle (fi_oracle.cpp, and fi_oracle_py.PyField where it has the call) reproduces every recorded bit: never skips;
  * with the live library: the fixture is what the script writes now, and 300 fresh seeded cases give equal bits;
  * tests/cxx/dump_rows.cpp, built against the drop-in and against the reference, writes byte-identical files.
Everything is compared as integers (rows, columns, counts, returns) or as the 32 bits of a float: no tolerance anywhere.
NaN, infinite and |coordinate| >= 2^31 positions are kept out (undefined behaviour in the reference, reference_rows.md)."""
import subprocess

import numpy as np
import pytest

import reference_rows as rr
from reference_rows import golden

CASES, UPSCALES = rr.fixture()
IDS = [c["name"] for c in CASES]


def _assert_same(got, want, what):
    for k in golden.OUTPUT_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, "%s: %s differs at %s (of %d): got %s, recorded %s" % (
            what, k, bad[:5], got[k].size, got[k][bad[:5]], want[k][bad[:5]])


class _PyBackend:
    """fi_oracle_py.PyField behind the method names run_case() uses (it has no error map)."""

    def __init__(self, oracle):
        from oracle import fi_oracle_py
        self.Weights = oracle.Weights
        py = fi_oracle_py

        class Field(py.PyField):
            num_rows = property(lambda s: len(s.rhs))
            num_triplets = property(lambda s: len(s.trip))
            get = py.PyField.arrays

            def error_map(s, x):
                return np.zeros(0, np.float32)

        self.LatticeField = Field


# ---- the oracle reproduces the fixture (never skips) -----------------------------------------------------------------------

def test_fixture_inputs_are_the_generators_and_cover_the_axes():
    """The committed inputs are what make_golden_reference.fixture_cases() makes today, and they hold what they are meant to."""
    made = golden.fixture_cases()
    assert [c["name"] for c in made] == IDS
    for m, c in zip(made, CASES):
        for k in golden.INPUT_KEYS:
            assert m[k].dtype == c[k].dtype and np.array_equal(m[k].view(np.uint8), c[k].view(np.uint8)), (c["name"], k)
    for (small, large, field), u in zip(golden.upscale_inputs(), UPSCALES):
        assert np.array_equal(small, u["small_sizes"]) and np.array_equal(large, u["large_sizes"])
        assert np.array_equal(field.view(np.uint32), u["field"].view(np.uint32))
    assert [(list(u["small_sizes"]), list(u["large_sizes"])) for u in UPSCALES] == golden.UPSCALES
    shapes = {tuple(c["sizes"]) for c in CASES}
    assert {tuple(s) for s in golden.NARROW + golden.REGULAR} <= shapes
    for D in (1, 2, 3):
        mine = [c for c in CASES if len(c["sizes"]) == D]
        assert {tuple(c["kernels"]) for c in mine} == set(golden.KERNEL_PAIRS)
        for j in range(2, 8):                      # each model term alone, and all of them together
            assert any(c["weights"][j] > 0 and np.count_nonzero(c["weights"][2:]) == 1 for c in mine), (D, j)
        assert any(np.all(c["weights"][2:] > 0) for c in mine)
        for op in (golden.OP_VALUE, golden.OP_VALUE_NEAREST, golden.OP_GRADIENT):
            ret = np.concatenate([c["returns"][c["op_kind"] == op] for c in mine])
            assert ret.any() and not ret.all(), (D, op)
    for c in CASES[1:]:
        p, n = c["op_pos"], c["sizes"].astype(np.float32)
        assert np.any(np.signbit(p) & (p == 0)) and np.any(p == 1e6) and np.any(p == -1e6)
        assert np.any(p == n - 0.5) and np.any(p == np.nextafter(n - np.float32(0.5), np.float32(-np.inf)))
        assert np.any(p == -0.5) and np.any(p == np.nextafter(np.float32(-0.5), np.float32(0)))
        assert np.any(p == 2.5) and np.any(p == -1.5) and np.any(p == n - 1)
        assert np.all(np.isfinite(p)) and np.abs(p).max() < 2.0 ** 31
        for arr in (c["op_weight"],) + ((c["pw"],) if len(c["pw"]) else ()):
            assert np.any(arr == 0) and np.any(arr < 0) and np.any(arr == np.float32(1e-30))
        assert np.any(c["op_grad"] == 0) and (len(c["nrm"]) == 0 or np.any(c["nrm"] == 0))
        assert set(c["op_kernel"]) == {0, 1, 2}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_reproduces_recorded_rows(oracle, case):
    _assert_same(golden.run_case(oracle, case), case, case["name"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_python_restatement_reproduces_recorded_rows(oracle, case):
    got = golden.run_case(_PyBackend(oracle), case)
    got["errmap"] = case["errmap"]                 # PyField has no generate_error_map
    _assert_same(got, case, case["name"])


def test_oracle_reproduces_recorded_upscales(oracle):
    for u in UPSCALES:
        got = oracle.upscale_field(u["field"], u["small_sizes"], u["large_sizes"])
        assert np.array_equal(got.view(np.uint32), u["out"]), (u["small_sizes"], u["large_sizes"])


# ---- the live library ----------------------------------------------------------------------------------------------------

def test_fixture_is_what_the_script_writes_now():
    rr.require_live_library()
    made = golden.generate(rr.fi_ref)
    z = np.load(golden.NPZ)
    assert sorted(made) == sorted(z.files)
    for k in z.files:
        assert made[k].dtype == z[k].dtype and np.array_equal(made[k], z[k]), k
    assert bytes(CASES[0]["text"]).decode().splitlines()[1] == "2 = 1 * x5"


def test_live_sweep_of_300_fresh_cases(oracle):
    rr.require_live_library()
    py = _PyBackend(oracle)
    rng = np.random.default_rng(4242)
    for seed in range(300):
        case = golden.sweep_case(seed)
        want = golden.run_case(rr.fi_ref, case)
        _assert_same(golden.run_case(oracle, case), want, "sweep case %d" % seed)
        if seed % 6 == 0:
            got = golden.run_case(py, case)
            got["errmap"] = want["errmap"]
            _assert_same(got, want, "sweep case %d (PyField)" % seed)
        D = int(rng.integers(1, 4))
        small, large = rng.integers(1, 7, D), rng.integers(1, 12, D)
        field = rng.normal(size=int(np.prod(small))).astype(np.float32)
        assert np.array_equal(oracle.upscale_field(field, small, large).view(np.uint32),
                              rr.fi_ref.upscale_field(field, small, large).view(np.uint32)), (seed, small, large)


def test_reference_checks_fail_where_the_oracle_refuses(oracle):
    """The abort conventions (field_interpolation.cpp:238, :361, :434): the logging stand-in throws, the oracle raises."""
    rr.require_live_library()
    pos, nrm = np.array([[1.0, 1.0]], np.float32), np.array([[1.0, 0.0]], np.float32)
    for mod, err in ((rr.fi_ref, rr.fi_ref.RefCheckFailed), (oracle, ValueError)):
        f = mod.LatticeField([4, 4])
        with pytest.raises(err):
            f.add_gradient_constraint(pos[0], nrm[0], 1.0, 7)
        with pytest.raises(err):
            f.add_points(1.0, 0, 1.0, 1, pos, None, None)          # nearest-neighbour value kernel without normals
        assert f.num_rows == 0 and f.num_triplets == 0
    with pytest.raises(rr.fi_ref.RefCheckFailed):
        rr.fi_ref.upscale_field(np.zeros(4, np.float32), [2, 2], [5])


# ---- the drop-in's host builders -------------------------------------------------------------------------------------------

def _run_dump(exe, tmp_path, tag):
    cases_file, out = str(tmp_path / "cases.txt"), str(tmp_path / (tag + ".txt"))
    rr.write_case_file(cases_file, CASES, UPSCALES)
    run = subprocess.run([exe, cases_file, out], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    return open(out, "rb").read()


def _assert_same_dump(got, want, who):
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        case = [line for line in w[:first + 1] if line.startswith(b"case ")][-1:]
        pytest.fail("%s at line %d (%s): got %r, expected %r" % (who, first, case, g[first:first + 1], w[first:first + 1]))


def test_dropin_host_builders_write_the_recorded_rows(tmp_path):
    """dump_rows built against include/ + libfield_interpolation.so writes, for every fixture case, exactly the rows, right-hand
    sides, returns and operator<< text the reference recorded.  Host code: no device is touched.  Never skips."""
    _assert_same_dump(_run_dump(rr.build_dropin_exe(), tmp_path, "dropin"), rr.expected_dump(CASES),
                      "the drop-in differs from the recorded rows")


def test_dropin_and_reference_programs_write_the_same_bytes(tmp_path):
    """The same source built twice -- against the drop-in, and against the reference's headers + libfi_ref.so -- two programs,
    so no symbol of one library meets the other's."""
    rr.require_live_library()
    _assert_same_dump(_run_dump(rr.build_dropin_exe(), tmp_path, "dropin"), _run_dump(rr.build_ref_exe(), tmp_path, "ref"),
                      "the drop-in differs from the reference program")
