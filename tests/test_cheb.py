"""The Chebyshev interval and recurrence of the solver's polynomials (field_interpolation_amd/csrc/fi_cheb.h) checked on the
host: tests/cxx/test_cheb.cpp is a program of its own -- no device, no Python in the process -- built with the address and
undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cheb_constants_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_cheb")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "field_interpolation_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "test_cheb.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all cheb checks passed" in r.stdout
