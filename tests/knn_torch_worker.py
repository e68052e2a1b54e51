"""Worker of tests/test_gpu_knn.py::test_device_tensors and tests/test_gpu_normals.py::test_device_tensors, started as a
fresh process: torch brings its own HIP runtime and must stay out of the pytest process.  The points, queries and
viewpoints of <in.npz> go to the device as torch tensors; the k-nearest and normal results of the context and of a
PointIndex come back to <out.npz>, with flags for where each output lived."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
a = np.load(src)
sizes = [int(s) for s in a["sizes"]]
k = int(a["k"][0])
pos = torch.from_numpy(a["pos"]).cuda()
q = torch.from_numpy(a["q"]).cuda()
view = torch.from_numpy(a["view"]).cuda()
f = fi.LatticeField(sizes)
f.add_field_constraints(fi.Weights())
f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, pos)
out = {}
d, i = f.knn(q, k)
out["on_device"] = np.array([d.is_cuda and i.is_cuda and i.dtype == torch.int64 and tuple(d.shape) == (q.shape[0], k)])
out["ctx_d"], out["ctx_i"] = d.cpu().numpy(), i.cpu().numpy()
out["ctx_d_only"] = f.knn(q, k, indices=False).cpu().numpy()
pi = fi.PointIndex(pos)
d, i = pi.knn(q, k)
out["pts_d"], out["pts_i"] = d.cpu().numpy(), i.cpu().numpy()
e = f.knn(torch.zeros((0, len(sizes)), device="cuda"), k)
out["empty_ok"] = np.array([tuple(e[0].shape) == (0, k) and tuple(e[1].shape) == (0, k) and e[0].is_cuda])
n, v = f.estimate_normals(k=k, viewpoints=view, variation=True)
out["normals_on_device"] = np.array([n.is_cuda and v.is_cuda])
out["ctx_n"], out["ctx_v"] = n.cpu().numpy(), v.cpu().numpy()
n, v = pi.estimate_normals(k=k, viewpoints=view, variation=True)
out["pts_n"], out["pts_v"] = n.cpu().numpy(), v.cpu().numpy()
n = pi.estimate_normals(k=k, device=True)
out["plain_on_device"] = np.array([n.is_cuda])
out["pts_n_plain"] = n.cpu().numpy()
np.savez(dst, **out)
print("knn torch worker done")
