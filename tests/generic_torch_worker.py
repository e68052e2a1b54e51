"""Worker of tests/test_gpu_generic_scale.py::test_device_memory_input_equals_host_memory_input, started as a fresh
process: torch brings its own HIP runtime and must stay out of the pytest process.  The batches of <in.npz> (r0, c0, v0, b0,
r1, ...) go to the device as torch tensors and into fi_add_rows_coo as FI_DEVICE memory; A^T b, diag and A^T A x (twice) of
an f32 and an f64 context come back in <out.npz>."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
a = np.load(src)
n, nb, x = int(a["n"]), int(a["nbatches"]), a["x"]
out = {}
for dtype in ("f32", "f64"):
    f = fi.LatticeField([n], dtype=dtype)
    f.add_field_constraints(fi.Weights(model_2=0.0))
    for k in range(nb):
        r, c, v, b = (torch.from_numpy(a["%s%d" % (name, k)]).cuda() for name in "rcvb")
        assert r.is_cuda and v.is_cuda and b.is_cuda and r.dtype == torch.int32 and v.dtype == torch.float32
        f.add_rows_coo(r, c, v, b)
    out["atb_" + dtype], out["diag_" + dtype] = f.Atb(), f.diag()
    out["y_" + dtype], out["y2_" + dtype] = f.apply_AtA(x), f.apply_AtA(x)
    out["rows_" + dtype] = np.array([f.stats()["num_generic_rows"]])
    try:                                                         # mixed memory is refused before anything is copied
        f.add_rows_coo(a["r0"], a["c0"], torch.from_numpy(a["v0"]).cuda(), a["b0"])
        out["mixed_refused_" + dtype] = np.array([False])
    except ValueError:
        out["mixed_refused_" + dtype] = np.array([True])
np.savez(dst, **out)
print("generic torch worker done")
