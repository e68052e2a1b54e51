"""Iso-contours over slabs: the pieces of a loop-back group (2, 3 and 4 slabs, 2-D and 3-D, a whole field and the members'
solutions) and of two processes on the host-staged test transport, merged by key, equal the undivided mesh exactly --
the same keys, bit-equal positions and normals, the same primitives in the same order."""
import os
import subprocess
import sys

import numpy as np
import pytest

import iso_reference as R
from util import sphere_points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _equal(a, b):
    assert np.array_equal(a.keys, b.keys)
    assert np.array_equal(a.indices, b.indices)
    assert np.array_equal(a.vertices.view(np.uint32), b.vertices.view(np.uint32))
    assert np.array_equal(a.normals.view(np.uint32), b.normals.view(np.uint32))


def _smooth(sizes, seed):
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sizes[::-1]], indexing="ij")
    f = np.zeros(g[0].shape)
    for _ in range(5):
        k = rng.normal(size=len(sizes)) * 0.35
        f += np.cos(sum(kk * gg for kk, gg in zip(k[::-1], g)) + rng.uniform(0, 6.3))
    return f.astype(np.float32).reshape(-1)


@pytest.mark.parametrize("nranks", [2, 3, 4])
@pytest.mark.parametrize("sizes", [[23, 19, 17], [41, 37]])
def test_group_pieces_of_a_whole_field(fi, sizes, nranks):
    f = _smooth(sizes, nranks)
    grp = fi.LatticeGroup(sizes, nranks)
    pieces = grp.iso_surface(f, 0.15)
    assert len(pieces) == nranks
    one = fi.iso_surface(f, sizes, 0.15)
    _equal(fi.merge_meshes(pieces), one)
    # every piece lists exactly the vertices its primitives use
    for p in pieces:
        assert np.array_equal(np.unique(p.indices), np.arange(len(p.keys)))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("nranks", [2, 3, 4])
@pytest.mark.parametrize("sizes", [[26, 24, 22], [48, 44]])
def test_group_pieces_of_the_solution(fi, sizes, nranks, dtype):
    rng = np.random.default_rng(7)
    pos, nrm = sphere_points(rng, sizes, 2000)
    w = fi.Weights()
    grp = fi.LatticeGroup(sizes, nranks, dtype=dtype)
    grp.add_field_constraints(w)
    grp.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
    grp.assemble()
    x, it, rel = grp.solve_cg(None, 0, 1e-6)
    pieces = grp.iso_surface()
    merged = fi.merge_meshes(pieces)
    _equal(merged, fi.iso_surface(x, sizes))
    v, n, idx, keys = R.extract(x, sizes)
    assert np.array_equal(merged.keys, keys) and np.array_equal(merged.indices, idx)


def test_group_halo_below_two_is_unsupported(fi):
    # model_1 alone reaches one plane: the slabs store one ghost plane, the pieces' normals need two
    sizes = [40, 36]
    pos, nrm = sphere_points(np.random.default_rng(5), sizes, 600)
    w = fi.Weights(model_1=0.5, model_2=0.0)
    grp = fi.LatticeGroup(sizes, 3)
    grp.add_field_constraints(w)
    grp.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
    grp.assemble()
    x, it, rel = grp.solve_cg(None, 0, 1e-5)
    with pytest.raises(fi.FiError) as e:
        grp.iso_surface()
    assert e.value.code == 5       # FI_ERR_UNSUPPORTED
    # the whole field handed in needs no exchange
    _equal(fi.merge_meshes(grp.iso_surface(x)), fi.iso_surface(x, sizes))


def test_two_processes(fi, tmp_path):
    out = str(tmp_path / "iso.npz")
    env = dict(os.environ, FI_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", FI_ISO_OUT=out,
               FI_HIP_LIB=os.path.join(ROOT, "field_interpolation_amd", "libfi_hip_test.so"))
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "iso_rank_worker.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = np.load(out)
    sizes = [int(s) for s in d["sizes"]]
    x = np.concatenate([d["x0"], d["x1"]])
    one = fi.iso_surface(x, sizes)
    for tag in ("a", "b"):
        pieces = [fi.IsoMesh(*[d["%s%d_%s" % (tag, r, k)] for k in ("vertices", "normals", "indices", "keys")]) for r in range(2)]
        _equal(fi.merge_meshes(pieces), one)
