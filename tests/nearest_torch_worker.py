"""Worker of tests/test_gpu_nearest.py::test_device_tensors, started as a fresh process: torch brings its own HIP runtime
and must stay out of the pytest process.  The points and queries of <in.npz> go to the device as torch tensors; the
context, PointIndex and distance-field results come back to <out.npz>, with flags for where each output lived."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
a = np.load(src)
sizes = [int(s) for s in a["sizes"]]
pos = torch.from_numpy(a["pos"]).cuda()
q = torch.from_numpy(a["q"]).cuda()
f = fi.LatticeField(sizes)
f.add_field_constraints(fi.Weights())
f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, pos)
out = {}
d, i = f.nearest(q, indices=True)
out["on_device"] = np.array([d.is_cuda and i.is_cuda and i.dtype == torch.int64])
out["ctx_d"], out["ctx_i"] = d.cpu().numpy(), i.cpu().numpy()
out["ctx_d_only"] = f.nearest(q).cpu().numpy()
pi = fi.PointIndex(pos)
d, i = pi.nearest(q, indices=True)
out["pts_d"], out["pts_i"] = d.cpu().numpy(), i.cpu().numpy()
d, i = f.distance_field(indices=True, device=True)
out["field_on_device"] = np.array([d.is_cuda and i.is_cuda])
out["ctx_fd"], out["ctx_fi"] = d.cpu().numpy(), i.cpu().numpy()
d, i = pi.distance_field(sizes, indices=True, device=True)
out["pts_fd"], out["pts_fi"] = d.cpu().numpy(), i.cpu().numpy()
e = f.nearest(torch.zeros((0, len(sizes)), device="cuda"), indices=True)
out["empty_ok"] = np.array([e[0].shape == (0,) and e[1].shape == (0,) and e[0].is_cuda])
np.savez(dst, **out)
print("nearest torch worker done")
