"""Point queries over slabs: a loop-back group (2, 3 and 4 slabs, 2-D and 3-D, fp32 and fp64, a whole field and the members'
solutions) and two processes on the host-staged test transport return, on every rank, results bit-identical to sampling
the undivided field -- with points on every seam plane and on either side of it."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import sample_reference as R
from util import sphere_points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _same(got, want):
    got = np.ascontiguousarray(got, np.float32).reshape(-1)
    want = np.ascontiguousarray(want, np.float32).reshape(-1)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def seam_points(rng, sizes, nranks, n=1500):
    """random points over the lattice (some outside), and points on every seam plane of the equal split and on either
    side of it, along the slowest axis"""
    D = len(sizes)
    G = sizes[-1]
    hi = np.array(sizes, np.float32) - 1
    p = (rng.uniform(-0.02, 1.02, size=(n, D)) * hi).astype(np.float32)
    seams = [r * G // nranks for r in range(1, nranks)] + [0, G - 1]
    extra = []
    for s in seams:
        for dz in (-1.0, -0.5, -1e-3, 0.0, 1e-3, 0.5, 1.0, 1.5):
            q = (rng.uniform(0, 1, size=(16, D)) * hi).astype(np.float32)
            q[:, D - 1] = np.float32(s + dz)
            q[::4, : D - 1] = np.round(q[::4, : D - 1])
            extra.append(q)
    p = np.concatenate([p] + extra)
    p[:3, D - 1] = [np.nan, -0.0, np.nextafter(hi[D - 1], np.float32(1e9))]
    return p


def _smooth(sizes, seed):
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sizes[::-1]], indexing="ij")
    f = np.zeros(g[0].shape)
    for _ in range(5):
        k = rng.normal(size=len(sizes)) * 0.35
        f += np.cos(sum(kk * gg for kk, gg in zip(k[::-1], g)) + rng.uniform(0, 6.3))
    return f.astype(np.float32).reshape(-1)


def _both(fi, got_fn, want_fn):
    for cubic in (False, True):
        gv, gg = got_fn(cubic)
        wv, wg = want_fn(cubic)
        _same(gv, wv)
        _same(gg, wg)


@pytest.mark.parametrize("nranks", [2, 3, 4])
@pytest.mark.parametrize("sizes", [[23, 19, 17], [41, 37]], ids=["3d", "2d"])
def test_group_whole_field(fi, sizes, nranks):
    f = _smooth(sizes, nranks)
    pos = seam_points(np.random.default_rng(nranks), sizes, nranks)
    grp = fi.LatticeGroup(sizes, nranks)
    _both(fi, lambda cubic: grp.sample(pos, f, gradients=True, cubic=cubic, fill=-3.0),
          lambda cubic: fi.sample_field(f, sizes, pos, gradients=True, cubic=cubic, fill=-3.0))
    # without gradients, and the oracle
    _same(grp.sample(pos, f, cubic=True), R.sample(f, sizes, pos, cubic=True))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("nranks", [2, 3, 4])
@pytest.mark.parametrize("sizes", [[26, 24, 22], [48, 44]], ids=["3d", "2d"])
def test_group_solution(fi, sizes, nranks, dtype):
    rng = np.random.default_rng(7)
    pts, nrm = sphere_points(rng, sizes, 2000)
    w = fi.Weights()
    grp = fi.LatticeGroup(sizes, nranks, dtype=dtype)
    grp.add_field_constraints(w)
    grp.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pts, nrm, None)
    grp.assemble()
    x, it, rel = grp.solve_cg(None, 0, 1e-6)
    pos = np.concatenate([seam_points(rng, sizes, nranks), pts])
    if dtype == "f32":   # the members' solution in place = the undivided field
        want = lambda cubic: fi.sample_field(x, sizes, pos, gradients=True, cubic=cubic)  # noqa: E731
    else:                # the fp64 solution, sampled in fp64
        x64 = grp.solution_f64()
        want = lambda cubic: R.sample(x64, sizes, pos, cubic=cubic, gradients=True, dtype=np.float64)  # noqa: E731
    _both(fi, lambda cubic: grp.sample(pos, gradients=True, cubic=cubic), want)
    # the whole lattice passed in (fp32) is sampled in fp32, in either dtype
    _same(grp.sample(pos, x, cubic=True), fi.sample_field(x, sizes, pos, cubic=True))


def test_group_one_ghost_plane(fi):
    # model_1 alone reaches one plane: the slabs store one ghost plane -- enough for linear, too few for cubic
    sizes = [40, 36]
    pts, nrm = sphere_points(np.random.default_rng(5), sizes, 600)
    w = fi.Weights(model_1=0.5, model_2=0.0)
    grp = fi.LatticeGroup(sizes, 3)
    grp.add_field_constraints(w)
    grp.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pts, nrm, None)
    grp.assemble()
    x, it, rel = grp.solve_cg(None, 0, 1e-5)
    pos = seam_points(np.random.default_rng(1), sizes, 3)
    _same(grp.sample(pos), fi.sample_field(x, sizes, pos))
    with pytest.raises(fi.FiError) as e:
        grp.sample(pos, cubic=True)
    assert e.value.code == 5       # FI_ERR_UNSUPPORTED
    # the whole field handed in needs no exchange
    _same(grp.sample(pos, x, cubic=True), fi.sample_field(x, sizes, pos, cubic=True))


def test_two_processes(fi, tmp_path):
    out = str(tmp_path / "sample.npz")
    env = dict(os.environ, FI_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", FI_SAMPLE_OUT=out,
               FI_HIP_LIB=os.path.join(ROOT, "field_interpolation_amd", "libfi_hip_test.so"))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "sample_rank_worker.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = np.load(out)
    sizes = [int(s) for s in d["sizes"]]
    x = np.concatenate([d["x0"], d["x1"]])
    pos = d["pos"]
    for cubic in (0, 1):
        wv, wg = fi.sample_field(x, sizes, pos, gradients=True, cubic=bool(cubic))
        for rank in (0, 1):
            for tag in ("a", "b"):   # a: the solution in place, b: the owned values passed in
                _same(d["%s%d_v%d" % (tag, rank, cubic)], wv)
                _same(d["%s%d_g%d" % (tag, rank, cubic)], wg)
