"""Worker of tests/test_gpu_mls.py::test_device_tensors, started as a fresh process: torch brings its own HIP runtime and
must stay out of the pytest process.  The cloud, the queries and the guide normals of <in.npz> go to the device as torch
tensors, through PointIndex / LatticeField smooth and project and through smooth_points; the answers come back to <out.npz>."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
a = np.load(src)
dev = {k: torch.from_numpy(a[k]).cuda() for k in a.files}
host = lambda x: x.cpu().numpy()  # noqa: E731
out, on_device = {}, []


def keep(name, got):
    on_device.extend(t.is_cuda for t in got)
    for i, t in enumerate(got):
        out["%s_%d" % (name, i)] = host(t)


field = fi.LatticeField([20, 18, 16])
field.add_field_constraints(fi.Weights())
field.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, dev["pos"])
for name, index in (("pts", fi.PointIndex(dev["pos"])), ("ctx", field)):
    keep(name + "_own", index.smooth(k=16, radius=2.5, max_move=0.5, normals=dev["g"], curvature=True, order=True))
    keep(name + "_ext", index.project(dev["q"], k=16, radius=2.5, degree=1, curvature=True, order=True))
keep("free", fi.smooth_points(dev["pos"], 2.5, k=16, max_move=0.5, normals=dev["g"], curvature=True, order=True))
# host normals with device=True: they are taken to the device
keep("mixed", fi.PointIndex(dev["pos"]).smooth(k=16, radius=2.5, max_move=0.5, normals=a["g"], curvature=True, order=True, device=True))
empty = fi.PointIndex(dev["pos"]).project(dev["q"][:0], radius=1.0, order=True)
on_device.append(all(t.is_cuda and t.shape[0] == 0 for t in empty))
out["on_device"] = np.array(on_device)
np.savez(dst, **out)
print("mls torch worker done")
