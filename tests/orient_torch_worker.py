"""Worker of tests/test_gpu_orient.py::test_device_tensors, started as a fresh process: torch brings its own HIP runtime and
must stay out of the pytest process.  The points, normals and the viewpoint of <in.npz> go to the device as torch tensors;
the oriented normals and components of the context and of a PointIndex come back to <out.npz>, with flags for where each
output lived and whether the input tensor was left alone."""
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
nrm = torch.from_numpy(a["nrm"]).cuda()
view = torch.from_numpy(a["view"]).cuda()
f = fi.LatticeField(sizes)
f.add_field_constraints(fi.Weights())
f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, pos)
out = {}
n, c = f.orient_normals(nrm, k=k, viewpoints=view, components=True)
on_device = [n.is_cuda and c.is_cuda and c.dtype == torch.int64 and tuple(n.shape) == tuple(nrm.shape)]
out["ctx_n"], out["ctx_c"] = n.cpu().numpy(), c.cpu().numpy()
pi = fi.PointIndex(pos)
n, c = pi.orient_normals(nrm, k=k, viewpoints=view, components=True)
on_device.append(n.is_cuda and c.is_cuda)
out["pts_n"], out["pts_c"] = n.cpu().numpy(), c.cpu().numpy()
n = pi.orient_normals(a["nrm"], k=k, viewpoints=a["view"], device=True)      # host arrays in, device=True
on_device.append(n.is_cuda)
out["host_guides_n"] = n.cpu().numpy()
n, c = pi.orient_normals(nrm, k=k, components=True)
on_device.append(n.is_cuda and c.is_cuda)
out["plain_n"], out["plain_c"] = n.cpu().numpy(), c.cpu().numpy()
out["on_device"] = np.array(on_device)
out["input_untouched"] = np.array([np.array_equal(nrm.cpu().numpy().view(np.uint32), a["nrm"].view(np.uint32))])
np.savez(dst, **out)
print("orient torch worker done")
