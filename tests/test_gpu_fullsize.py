"""BASELINE.json configurations at FULL size on one MI355X, checked through size-independent properties
(the oracle cannot solve these sizes in test time): verified residual b - A x, symmetry and bitwise
reproducibility of the operator, the physical meaning of the field (signed distance near the surface),
slab decomposition equal to the undivided solve.  fp64 contexts where the tolerance (1e-5 / 1e-6 true
residual on systems with kappa ~ side^4) is out of fp32's reach -- SURVEY.md section 7, hard part 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fi():
    import field_interpolation_amd as fi
    from field_interpolation_amd import _capi
    assert _capi.device_count() >= 1
    return fi


def _symmetry_and_determinism(f, n, seed=0):
    rng = np.random.default_rng(seed)
    x, y = rng.normal(size=n), rng.normal(size=n)
    Ax, Ay = f.apply_AtA(x), f.apply_AtA(y)
    assert abs(y @ Ax - x @ Ay) <= 1e-9 * abs(y @ Ax)            # A^T A is symmetric
    assert x @ Ax > 0                                             # and positive
    np.testing.assert_array_equal(Ax, f.apply_AtA(x))             # bitwise reproducible
    Axy = f.apply_AtA(2.0 * x - 3.0 * y)
    assert np.abs(Axy - (2.0 * Ax - 3.0 * Ay)).max() <= 1e-9 * np.abs(Ax).max()   # linear


def test_config2_1024x1024_noisy_values(fi):
    """2D 1024x1024, 10k random noisy value constraints + smoothness prior (model_2 = 10)."""
    from field_interpolation_amd import synth
    sizes, w, pos, val = synth.config2()
    from field_interpolation_amd import bench_settings as bs
    f = bs.headline_field(fi, 2, sizes, w)           # bench.py --config 2's settings
    f.add_points(w.data_pos, w.value_kernel, 0.0, w.gradient_kernel, pos, None, None, values=val)
    f.assemble()
    assert f.stats()["num_data_rows"] == 10000
    _symmetry_and_determinism(f, 1024 * 1024)
    x, it, rel = f.solve_cg(None, 2000, 1e-5)
    st = f.stats()
    assert st["converged"] == 1 and st["verified_residual"] <= 1e-5 and f.true_residual() <= 1.01e-5
    # a smooth field through noisy data: it tracks the noise-free signal better than the noisy samples do
    u, v = pos[:, 0] / 1023.0, pos[:, 1] / 1023.0
    truth = 0.5 * np.sin(10.0 * u * (1.0 + 2.0 * u)) * np.cos(7.0 * v)
    ix, iy = np.round(pos[:, 0]).astype(int), np.round(pos[:, 1]).astype(int)
    fitted = x.reshape(1024, 1024)[iy, ix]
    assert np.sqrt(np.mean((fitted - truth) ** 2)) < np.sqrt(np.mean((val - truth) ** 2))


def test_config3_4096x4096_sdf_from_oriented_points(fi):
    """2D 4096x4096 SDF from 200k oriented point-cloud samples (value + gradient rows)."""
    from field_interpolation_amd import synth
    sizes, w, pos, nrm = synth.config3()
    from field_interpolation_amd import bench_settings as bs
    f = fi.sdf_from_points(sizes, w, pos, nrm, dtype="f64")
    bs.configure(f, bs.SETTINGS[3]["levels"], bs.SETTINGS[3]["coarse_tol"], kcycle=bs.SETTINGS[3].get("kcycle", 0), cheb=bs.SETTINGS[3].get("cheb"))   # bench.py --config 3's settings
    f.assemble()
    assert f.stats()["num_data_rows"] == 3 * 200000
    x, it, rel = f.solve_cg(None, 3000, 1e-5)
    st = f.stats()
    assert st["converged"] == 1 and f.true_residual() <= 1.01e-5
    field = x.reshape(4096, 4096)
    c = 0.5 * 4095
    assert field[int(c), int(c + 0.05 * 4095)] > 0        # inside the inverted circle (r = 0.1): outside the shape
    assert field[int(c), int(c + 0.2 * 4095)] < 0         # between circle and triangle: inside
    # "only accurate near field = 0" (field_interpolation.hpp:165): 80 lattice units (4 sigma of the sample noise)
    # off the surface along the normals the sign is right for nearly every sample; far from the data a 1e-5
    # residual pins nothing (the corner value still moves by O(10) between 1e-5 and 1e-7)
    unit = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    for sgn in (+1.0, -1.0):
        q = pos[::50] + sgn * 80.0 * unit[::50]
        ok = (q >= 0).all(1) & (q <= 4094).all(1)
        v = field[np.round(q[ok, 1]).astype(int), np.round(q[ok, 0]).astype(int)]
        assert np.mean(np.sign(v) == sgn) > 0.9          # (triangle corners and the noise tail make up the rest)


def test_config4_256cubed_bench_workload(fi):
    """3D 256^3, 1M scattered value constraints with bench.py's own solver settings: fp32, coarse-to-fine start over ONE
    coarser level, CG preconditioned by the 4-term Chebyshev polynomial (ratio 30), tol 1e-5 -- and bench.py's accurate
    leg on the same inputs (fp64 CG + fp32 V-cycle over 3 coarser levels to 1e-7): the two fields agree to what the
    1e-5 residual pins."""
    from field_interpolation_amd import synth
    sizes, w, pos, val = synth.config4()
    f = fi.LatticeField(sizes, dtype="f32")
    f.add_field_constraints(w)
    f.set_levels(1, 1e-5)
    f.set_polynomial(4, 30.0)
    f.add_points(w.data_pos, w.value_kernel, 0.0, w.gradient_kernel, pos, None, None, values=val)
    f.assemble()
    st = f.stats()
    assert st["num_data_rows"] == 1000000 and st["num_levels"] == 2
    x, it, rel = f.solve_cg(None, 0, 1e-5)
    st = f.stats()
    assert st["converged"] == 1 and st["verified_residual"] <= 1e-5
    assert abs(it - 15) <= 2, it                      # bench.py: 15 outer iterations (17 on the coarser level)
    from field_interpolation_amd import bench_settings as bs
    a = bs.headline_field(fi, 4, sizes, w, by_field=True)   # bench.py's headline solver, its settings, its stop rule (by the field)
    a.add_points(w.data_pos, w.value_kernel, 0.0, w.gradient_kernel, pos, None, None, values=val)
    a.assemble()
    xa, ita, rela = a.solve_cg(None, 0, bs.SETTINGS[4]["tol"])
    sta = a.stats()
    assert sta["converged"] == 1 and 0 <= sta["field_estimate"] <= bs.FIELD_TOLERANCE and a.true_residual() <= 3e-7
    assert 5 <= ita <= 8, ita                         # bench.py: 6-7 iterations (5 at the residual rounds 4-5 had calibrated)
    assert np.abs(x - xa).max() <= 5e-3 * np.abs(xa).max()   # the fp32 field at a 1e-5 residual: 2e-3 (bench: solution_rel_err)
    del a
    # the field is the (noisy) signed distance to the sphere, smoothed: check it on the lattice
    z, y, xx = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij")
    d = np.sqrt((xx - 127.5) ** 2 + (y - 127.5) ** 2 + (z - 127.5) ** 2) - 0.3 * 255
    err = x.reshape(256, 256, 256) - d
    inner = (slice(8, -8),) * 3
    assert np.abs(err[inner]).mean() < 0.15 and np.abs(err[inner]).max() < 2.0


def test_config4_slabs_equal_undivided_at_128cubed(fi):
    """3D lattice domain-split across 4 slabs (loop-back group = the RCCL path's kernels and rules)."""
    from field_interpolation_amd import synth
    sizes, w, pos, val = synth.config4(side=128, num_points=125000)
    one = fi.LatticeField(sizes, dtype="f32")
    grp = fi.LatticeGroup(sizes, 4, dtype="f32")
    for f in (one, grp):
        f.add_field_constraints(w)
        f.set_levels(2, 1e-4)
        f.add_points(w.data_pos, w.value_kernel, 0.0, w.gradient_kernel, pos, None, None, values=val)
        f.assemble()
    x1, it1, r1 = one.solve_cg(None, 0, 1e-5)
    xg, itg, rg = grp.solve_cg(None, 0, 1e-5)
    assert abs(it1 - itg) <= 5 and r1 <= 1e-5 and rg <= 1e-5
    assert np.abs(xg - x1).max() <= 2e-3 * np.abs(x1).max()
    assert grp.true_residual() <= 1.5e-5


def test_config5_512cubed_sdf_tol_1e6(fi):
    """3D 512^3 SDF from 5M oriented points, CG to 1e-6 with bench.py --config 5's settings (fp64 CG, fp32 K-cycle over 6
    coarser levels): verified residual, the bench's iteration count, and the meaning of the result -- a signed distance
    near the sphere."""
    from field_interpolation_amd import synth
    sizes, w, pos, nrm = synth.config5()
    from field_interpolation_amd import bench_settings as bs
    f = fi.sdf_from_points(sizes, w, pos, nrm, dtype="f64")
    bs.configure(f, bs.SETTINGS[5]["levels"], bs.SETTINGS[5]["coarse_tol"], kcycle=bs.SETTINGS[5].get("kcycle", 0), cheb=bs.SETTINGS[5].get("cheb"))   # bench.py --config 5: fp64 CG, fp32 K-cycle, 6 levels to 1e-2
    f.assemble()
    st = f.stats()
    assert st["num_data_rows"] == 4 * 5000000 and st["num_levels"] == 7
    x, it, rel = f.solve_cg(None, 1000, 1e-6)
    st = f.stats()
    assert st["converged"] == 1 and st["verified_residual"] <= 1e-6
    assert abs(it - 9) <= 3, it                      # (round 5's V-cycle, smoother of degree 4 over [l / 10, l]: 24; round 6's, 5 over [l / 40, l]: 20; the K-cycle on four levels: 9)
    field = x.reshape(512, 512, 512)
    c, R = 255.5, 0.3 * 511
    # "only accurate near field = 0" (field_interpolation.hpp:165): a signed distance close to the surface,
    # the right sign and monotone away from it
    prev = None
    for r_off in (-8.0, -4.0, -2.0, 0.0, 2.0, 4.0, 8.0):          # along +x through the centre
        ix = int(round(c + R + r_off))
        v = float(field[255, 255, ix])
        if abs(r_off) <= 2.0:
            assert abs(v - ((ix - c) - R)) < 0.6, (r_off, v)
        assert prev is None or v > prev
        prev = v
    assert field[255, 255, 255] < 0 and field[5, 5, 5] > 0


def test_config3_mixed_precision_equals_fp64(fi):
    """Config 3 with FI_OPT_MIXED_PRECISION (fp64 CG, fp32 V-cycle): the same verified fp64 residual and the same
    field as the pure fp64 solve, in about the same number of iterations.  Compared at 1e-8: at 1e-5 the field
    far from the data is not pinned yet (kappa ~ side^4) and two correct solves differ there by O(10)."""
    from field_interpolation_amd import synth
    sizes, w, pos, nrm = synth.config3()
    out = []
    for mixed in (False, True):
        f = fi.sdf_from_points(sizes, w, pos, nrm, dtype="f64")
        f.set_levels(7, 1e-4)
        f.set_multigrid(True)
        f.set_mixed_precision(mixed)
        f.assemble()
        x, it, rel = f.solve_cg(None, 3000, 1e-8)
        assert f.stats()["converged"] == 1 and f.true_residual() <= 1.01e-8
        out.append((x, it))
        del f
    (x0, it0), (x1, it1) = out
    assert abs(it1 - it0) <= it0 // 4      # measured: 198 / 199 (fp64, fused / unfused smoother) against 239 / 236 (mixed)
    assert np.abs(x1 - x0).max() <= 0.05 * np.abs(x0).max()


def test_config5_over_eight_slabs_keeps_all_levels(fi):
    """Config 5 over 8 slabs of 64 planes (the loop-back group: the RCCL path's kernels, geometry and ownership rules): the
    slab decomposition carries the levels down to 32^3 (4 planes per slab); 16^3 and 8^3 are the replicated tail.  All 6
    coarser levels exist and the solve takes the undivided solve's iterations (20) -- cut at 32^3 it would take twice as many
    (bench.py --config 5 --levels 4, measured with round 5's smoother: 51 against 25)."""
    from field_interpolation_amd import synth
    sizes, w, pos, nrm = synth.config5()
    grp = fi.LatticeGroup(sizes, 8, dtype="f64")
    grp.add_field_constraints(w)
    grp.set_levels(6, 1e-4)
    grp.set_multigrid(True)
    grp.set_mixed_precision(True)
    grp.add_points(w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, pos, nrm, None)
    grp.assemble()
    assert grp.stats()["num_levels"] == 7
    x, it, rel = grp.solve_cg(None, 1000, 1e-6)
    assert rel <= 1e-6 and grp.true_residual() <= 1.5e-6
    assert abs(it - 20) <= 3, it


def test_bench_line_contract_single_gpu():
    """The one JSON line of bench.py --full at N = 1 (a reduced lattice so that the CPU baseline takes seconds): every field
    of the measurement contract, the `roofline*` and `cpu_baseline` objects included; the headline is the solver that meets
    the field tolerance (fp64 CG + fp32 V-cycle), the fp32 residual-1e-5 mode sits in `fast`; and the cold figures."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--side", "96", "--cpu-side", "32",
                        "--full"],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["vs_baseline"] is None and d["dtype"] == "f64" and d["data"] == "synthetic" and d["unit"] == "lattice points/s"
    assert d["scaling"] == "strong"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 96 ** 3 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) <= 1e-9 and 0 < rf["frac"] < 1
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0
    for name in ("roofline_apply", "roofline_assembly"):
        assert d[name]["bound"] == "hbm" and 0 < d[name]["frac"] < 1 and d[name]["algorithmic_bytes"] > 0, name
    assert "double" in d["roofline_apply"]["kernel"]
    assert d["config"]["true_rel_residual"] <= 1e-6 and "V-cycle PCG" in d["config"]["solver"]
    # one stop rule for every workload (round 6): by the field, the solver's own estimate within the tolerance
    assert "by the field" in d["config"]["stop_rule"] and 0 <= d["config"]["field_estimate"] <= 1e-5
    assert 0 < d["host_io"]["ms_per_step"] and d["host_io"]["d2h_bytes"] == 4 * 96 ** 3
    # the headline meets the north-star's field tolerance (here against an fp64 GPU solve: the oracle's committed sample
    # covers 256^3 -- tests/test_gpu_fullsize_golden.py), the fast mode does not claim to
    assert d["solution_rel_err"] <= 1e-5 and d["config"]["field_tolerance_met"] is True
    assert d["fast"]["dtype"] == "f32" and d["fast"]["value"] > 0 and d["fast"]["true_rel_residual"] <= 1.5e-5
    assert d["fast"]["solution_rel_err"] > d["solution_rel_err"]
    assert d["cold_ms_per_step"] > 0 and d["cold_pooled_ms_per_step"] > 0


def test_bench_plain_line_single_gpu(tmp_path):
    """A plain run of bench.py (no --full) at N = 1: the headline fields of the contract, the figures of the timed region,
    the outputs of the last timed step, and none of what takes runs of its own."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--side", "96",
                        "--dump-outputs", out], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config",
              "roofline", "roofline_apply", "roofline_assembly"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["unit"] == "lattice points/s" and d["metric"].startswith("solved lattice points/sec")
    assert abs(d["value"] - 96 ** 3 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert "V-cycle PCG" in d["config"]["solver"] and d["config"]["true_rel_residual"] <= 1e-6
    for k in ("solution_rel_err", "fast", "calibrated_residual_r5", "cold_ms_per_step", "cold_pooled_ms_per_step", "host_io",
              "roofline_512", "cpu_baseline", "cpu_best_effort"):
        assert k not in d, k
    assert "solution_check" not in d["config"] and "field_tolerance_met" not in d["config"]
    x = np.load(os.path.join(out, "solution.npy"))
    assert x.dtype == np.float32 and x.shape == (96 ** 3,) and np.isfinite(x).all()
    assert int(np.load(os.path.join(out, "iterations.npy"))) == d["config"]["iterations"]
    assert float(np.load(os.path.join(out, "rel_residual.npy"))) == d["config"]["rel_residual"]
