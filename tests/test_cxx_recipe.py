"""The note beside a LinearEquation's rows (LinearEquation::recipe, field_interpolation_amd/cxx/recipe.hpp) and the
matrix-free path the drop-in's solvers take on its word: tests/cxx/test_recipe.cpp checks the note's validation on the
host (every in-place edit of a noted range is refused) and, on the GPU box, every solver entry point against an fp64
reference of the triplets in `eq` as they stand."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
EXE = os.path.join(ROOT, "tests", "cxx", "test_recipe")
_built = []


def _build():
    if not _built:
        subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
        subprocess.check_call(["g++", "-O1", "-std=c++14", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(PKG, "cxx"),
                               os.path.join(ROOT, "tests", "cxx", "test_recipe.cpp"), "-o", EXE,
                               "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-Wl,-rpath," + PKG,
                               "-Wl,-rpath,/opt/rocm/lib"])
        _built.append(EXE)
    return EXE


def _run(args, last_line):
    exe = _build()
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode != 3, "the test's own reference did not converge:\n" + out.stdout + out.stderr
    assert out.returncode == 0, out.stdout + out.stderr
    assert last_line in out.stdout


def _need_library():
    if not os.path.exists(os.path.join(PKG, "libfi_hip.so")):
        pytest.skip("libfi_hip.so not built")


@pytest.mark.parametrize("field", ["2d", "3d", "hand"])
def test_recipe_validation_refuses_every_edit(field):
    """B: host only -- the program starts and runs these checks on a machine without a device."""
    _need_library()
    _run(["host", field], "all host checks passed")


@pytest.mark.parametrize("args", [["sizing"], ["c1", "1", "references"], ["c1", "2", "references"],
                                  ["c1", "3", "references"]], ids=lambda a: "-".join(a))
def test_recipe_references_certify(args):
    """The host halves of C1 and C2: every reference passes its certificate, every C2 edit is large enough."""
    _need_library()
    _run(args, "all sizing checks passed" if args[0] == "sizing" else "all c1 references certified")


@pytest.mark.gpu
@pytest.mark.parametrize("args", [["c1", "1"], ["c1", "2"], ["c1", "3"], ["c2"], ["c3"]], ids=lambda a: "-".join(a))
def test_recipe_solvers_equal_the_reference(args):
    _run(args, "all %s checks passed" % args[0])
