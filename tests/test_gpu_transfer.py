"""Every grid-transfer kernel of field_interpolation_amd/csrc/fi_transfer.hip against a reference of the same operation, path by
path.  tests/cxx/test_transfer.hip is the program: it calls fi::launch_prolong, fi::launch_prolong_cubic and fi::launch_restrict
of the shipped libfi_hip.so directly, with hand-filled level pairs, and compares with dense per-axis matrices written from the
lattices' geometry (R = P^T, tensor products, fp64).  Integer inputs must come back as the reference's very numbers, in fp32 and
fp64; everything else within k u sum|w||x|; what a kernel does not own keeps a NaN pattern.  No solve is involved.

PLAN below is the list of cases with the kernel the dispatch must pick for each: the program restates the launchers' thresholds,
this file states the outcome shape by shape."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "field_interpolation_amd")
CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(ROOT, "tests", "cxx", "test_transfer.hip")
EXE = os.path.join(ROOT, "tests", "cxx", "test_transfer")
LIB = os.path.join(PKG, "libfi_hip.so")
GROUPS = ("prolong", "cubic", "restrict", "slabs")

LAUNCHERS = (
    "void fi::launch_prolong<float>(",
    "void fi::launch_prolong<double>(",
    "void fi::launch_prolong_cubic<float, float>(",
    "void fi::launch_prolong_cubic<double, double>(",
    "void fi::launch_prolong_cubic<float, double>(",
    "void fi::launch_restrict<float>(",
    "void fi::launch_restrict<double>(",
)


def _halvings(nf):
    """The halvings a small shape is run with: the hierarchy's own (even extents cell-centred), every axis vertex-centred, and
    only the slowest axis vertex-centred -- without repeats."""
    out = [[int(n % 2 == 0) for n in nf]]
    for cc in ([0] * len(nf), out[0][:-1] + [0]):
        if cc not in out:
            out.append(cc)
    return out


def _plan():
    plan = {g: [] for g in GROUPS}

    def add(group, op, kernels, nf, cc=None, ranks=1, switch="-"):
        cc = [int(n % 2 == 0) for n in nf] if cc is None else cc
        fmt = lambda v: "[" + ",".join(str(k) for k in v) + "]"  # noqa: E731
        plan[group].append((op, kernels, fmt(nf), fmt(cc), str(ranks), switch))

    def small(group, op, kernels, nf):
        for cc in _halvings(nf):
            add(group, op, kernels, nf, cc)

    big = ([256, 128, 128], [264, 132, 130])
    for nf in ([17], [16], [30]):
        small("prolong", "prolong", "k_prolong", nf)
    for nf in ([17, 16], [16, 18], [33, 19], [30, 22]):
        small("prolong", "prolong", "k_prolong2", nf)
    for nf in ([17, 16, 19], [16, 16, 16], [21, 18, 16]):
        small("prolong", "prolong", "k_prolong3", nf)
    for nf in big:
        add("prolong", "prolong", "k_prolong3_rows", nf)
        add("prolong", "prolong", "k_prolong3", nf, switch="FI_BLOCK_PROLONG")

    for nf in ([17, 16, 19], [16, 16, 16], [31, 22, 17]):
        small("cubic", "cubic", "k_prolong3_cubic", nf)
    for nf in big:
        add("cubic", "cubic", "k_prolong3_cubic_rows", nf)
        add("cubic", "cubic", "k_prolong3_cubic", nf, switch="FI_BLOCK_PROLONG")

    for nf in ([17], [16], [30]):
        small("restrict", "restrict", "k_restrict", nf)
    small("restrict", "restrict", "k_restrict2", [30, 17])
    for nf in ([64, 30], [130, 67]):
        add("restrict", "restrict", "k_restrict3_xy_tiled", nf)
        add("restrict", "restrict", "k_restrict2", nf, switch="FI_FLAT_RESTRICT")
    for nf in ([17, 16, 19], [16, 16, 16]):
        small("restrict", "restrict", "k_restrict3", nf)
    z, z4 = "+k_restrict3_z", "+k_restrict3_z4"
    for nf, two_pass in (([30, 17, 19], "k_restrict3_xy" + z), ([65, 30, 17], "k_restrict3_xy_tiled" + z),
                         ([66, 30, 16], "k_restrict3_xy_tiled" + z), ([64, 16, 17], "k_restrict3_xy_rows" + z),
                         ([136, 36, 16], "k_restrict3_xy_rows" + z), ([128, 128, 128], "k_restrict3_xy_rows" + z4),
                         ([128, 128, 127], "k_restrict3_xy_rows" + z4)):
        add("restrict", "restrict", two_pass, nf)
        add("restrict", "restrict", "k_restrict3", nf, switch="FI_ONE_PASS_RESTRICT")
        if nf[0] in (64, 136):
            add("restrict", "restrict", "k_restrict3_xy_tiled" + z, nf, switch="FI_TILED_RESTRICT")
            add("restrict", "restrict", "k_restrict3_xy" + z, nf, switch="FI_FLAT_RESTRICT")

    for nf, xy in (([16, 18, 40], "k_restrict3_xy"), ([17, 16, 41], "k_restrict3_xy"), ([40, 64], None),
                   ([64, 16, 48], "k_restrict3_xy_rows")):
        for ranks in (2, 3):
            if len(nf) == 2:
                add("slabs", "prolong", "k_prolong2", nf, ranks=ranks)
                add("slabs", "restrict", "k_restrict2", nf, ranks=ranks)
                continue
            add("slabs", "prolong", "k_prolong3", nf, ranks=ranks)
            add("slabs", "cubic", "k_prolong3_cubic", nf, ranks=ranks)
            add("slabs", "restrict", "k_restrict3", nf, ranks=ranks)
            add("slabs", "restrict", xy + z, nf, ranks=ranks)
    return plan


PLAN = _plan()
KERNELS = {"k_prolong", "k_prolong2", "k_prolong3", "k_prolong3_rows", "k_prolong3_cubic", "k_prolong3_cubic_rows", "k_restrict",
           "k_restrict2", "k_restrict3", "k_restrict3_xy", "k_restrict3_xy_tiled", "k_restrict3_xy_rows", "k_restrict3_z",
           "k_restrict3_z4"}
LINE = re.compile(r"^(plan|case) (\w+) op=(\w+) kernels=(\S+) nf=(\S+) cc=(\S+) ranks=(\d+) switch=(\S+)", re.M)


def _cases(text, word, group):
    """The cases of one group a run printed, in order, each once (a case is run in several precisions, inputs and modes)."""
    out = []
    for m in LINE.finditer(text):
        if m.group(1) == word and m.group(2) == group and (not out or out[-1] != m.groups()[2:]):
            out.append(m.groups()[2:])
    return out


def _build():
    deps = [SRC, LIB] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(EXE) and os.path.getmtime(EXE) >= max(os.path.getmtime(p) for p in deps):
        return EXE
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", CSRC,
                           "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE, "-L", PKG, "-lfi_hip", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_plan_names_every_transfer_kernel():
    named = set()
    for group in GROUPS:
        for case in PLAN[group]:
            named.update(case[1].split("+"))
    assert named == KERNELS


def test_transfer_program_builds_and_the_reference_holds():
    if not os.path.exists(LIB):
        pytest.skip("libfi_hip.so not built")
    exe = _build()
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", LIB], text=True)
    for name in LAUNCHERS:
        assert name in syms, name
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all host checks passed" in r.stdout
    for group in GROUPS:
        assert _cases(r.stdout, "plan", group) == PLAN[group], group


@pytest.mark.gpu
def test_transfer_kernels_equal_the_reference_on_every_path():
    exe = _build()
    for group in GROUPS:  # one fresh process per group; the first that fails ends the test
        r = subprocess.run([exe, group], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, "group %s:\n%s" % (group, (r.stdout + r.stderr)[-4000:])
        assert "all %s checks passed" % group in r.stdout
        assert _cases(r.stdout, "case", group) == PLAN[group], group
        print("\n".join(line for line in r.stdout.splitlines() if line.startswith("ratio ")))
