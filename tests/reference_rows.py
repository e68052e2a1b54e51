"""Shared by test_reference_rows.py and test_gpu_reference_rows.py: the recorded fixture of the reference's own compiled
assembly (tests/golden/reference_rows.npz, keys in reference_rows.md), the case file tests/cxx/dump_rows.cpp reads, the text it
has to write, and the two builds of that program."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "field_interpolation_amd")
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_reference as golden  # noqa: E402

from oracle import fi_ref  # noqa: E402

EXE_DROPIN = os.path.join(HERE, "cxx", "dump_rows_dropin")
EXE_REF = os.path.join(HERE, "cxx", "dump_rows_ref")
SRC = os.path.join(HERE, "cxx", "dump_rows.cpp")

_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = golden.load()
    return _FIXTURE


def require_live_library():
    """The live legs skip only where neither the library nor the reference's sources exist; sources without a library mean
    build() did not do its work."""
    import pytest
    if fi_ref.available():
        return
    if fi_ref.reference_present():
        pytest.fail("the reference's sources are at %s but oracle/_ref/libfi_ref.so is missing: run build()"
                    % fi_ref.reference_dir())
    pytest.skip("neither oracle/_ref/libfi_ref.so nor the reference's sources are here")


def _hex(a):
    return " ".join("%08x" % b for b in np.ascontiguousarray(a, np.float32).ravel().view(np.uint32))


def write_case_file(path, cases, upscales):
    lines = [str(len(cases))]
    for c in cases:
        D = len(c["sizes"])
        lines.append("%s %d %s %s %d %d %d %d" % (c["name"], D, " ".join(map(str, c["sizes"])), _hex(c["weights"]),
                                                  c["kernels"][0], c["kernels"][1], c["flags"][0], c["flags"][1]))
        lines.append("%d %d %d %s %s %s" % (len(c["pos"]), len(c["nrm"]) > 0, len(c["pw"]) > 0, _hex(c["pos"]), _hex(c["nrm"]),
                                            _hex(c["pw"])))
        lines.append(str(len(c["op_kind"])))
        for k in range(len(c["op_kind"])):
            lines.append("%d %d %s %s %s %s" % (c["op_kind"][k], c["op_kernel"][k], _hex(c["op_pos"][k]), _hex(c["op_grad"][k]),
                                                _hex(c["op_value"][k]), _hex(c["op_weight"][k])))
        lines.append("%d %s" % (len(c["x"]), _hex(c["x"])))
    lines.append(str(len(upscales)))
    for u in upscales:
        lines.append("%d %s %s %s" % (len(u["small_sizes"]), " ".join(map(str, u["small_sizes"])),
                                      " ".join(map(str, u["large_sizes"])), _hex(u["field"])))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def expected_dump(cases):
    """What dump_rows (without --device) has to write for the recorded rows, byte for byte."""
    out = []
    for c in cases:
        out.append("case %s\ncounts %d %d\n" % (c["name"], c["counts"][0], c["counts"][1]))
        out.extend("t %d %d %08x\n" % t for t in zip(c["rows"], c["cols"], c["vals"]))
        out.append("rhs %d%s\n" % (len(c["rhs"]), "".join(" %08x" % b for b in c["rhs"])))
        out.append("returns %d%s\n" % (len(c["returns"]), "".join(" %d" % r for r in c["returns"])))
        if c["flags"][1]:
            out.append("text %d\n%s" % (len(c["text"]), bytes(c["text"]).decode()))
    return "".join(out).encode()


def parse_device_dump(text):
    """-> (error map bits per case, upscaled bits per pair, GpuLatticeField's returns per case) from dump_rows --device."""
    maps, ups, rets = [], [], []
    for line in text.splitlines():
        tok = line.split()
        if tok and tok[0] == "gpureturns":
            rets.append(np.array(tok[2:], np.uint8))
            assert len(rets[-1]) == int(tok[1])
        if tok and tok[0] in ("errmap", "upscale"):
            bits = np.array([int(t, 16) for t in tok[2:]], np.uint32)
            assert len(bits) == int(tok[1])
            (maps if tok[0] == "errmap" else ups).append(bits)
    return maps, ups, rets


def build_dropin_exe():
    """dump_rows against include/ and libfield_interpolation.so."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "cxx")])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE_DROPIN,
                           "-L", PKG, "-lfield_interpolation", "-lfi_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE_DROPIN


def build_ref_exe():
    """dump_rows against the reference's headers and oracle/_ref/libfi_ref.so; where the sources are not here (a machine the
    built tree was copied to), the program built beside the library is used as it is."""
    ref = os.path.dirname(fi_ref.SO)
    if fi_ref.reference_present():
        subprocess.check_call(["g++", "-O1", "-std=c++14", "-I", fi_ref.reference_dir(), SRC, "-o", EXE_REF,
                               "-L", ref, "-lfi_ref", "-Wl,-rpath," + ref])
    elif not os.path.exists(EXE_REF):
        import pytest
        pytest.skip("oracle/_ref/libfi_ref.so is here, but neither the reference's headers nor a built dump_rows_ref")
    return EXE_REF
