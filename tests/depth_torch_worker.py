"""Worker of tests/test_gpu_depth.py::test_device_tensors, started as a fresh process: torch brings its own HIP runtime and
must stay out of the pytest process.  The depth and incidence images and the image weights of <in.npz> go to the device as
torch tensors, through DepthVolume (integrate, tsdf, weight, constraints, load), depth_to_points and LatticeField.add_volume;
the answers come back to <out.npz>."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
a = np.load(src)
cams = [fi.Camera(p, *k, int(s[0]), int(s[1]), "z" if s[2] == 0 else "range") for p, k, s in zip(a["pose"], a["intr"], a["shape"])]
depths, incs, weights = (torch.from_numpy(a[k]).cuda() for k in ("depths", "incs", "weights"))
host = lambda x: x.cpu().numpy()  # noqa: E731
out, on_device = {}, []

sizes = [20, 18, 16]
vol = fi.DepthVolume(sizes, 2.5, 4.0)
vol.integrate(cams, depths, incs, weights, min_incidence=0.3)
t, W = vol.tsdf(device=True), vol.weight(device=True)
on_device += [t.is_cuda, W.is_cuda]
out["tsdf"], out["weight"] = host(t), host(W)
# the state through load, from device tensors, into a second volume: the constraints come from that one
again = fi.DepthVolume(sizes, 2.5, 4.0).load(t, W)
con = again.constraints(1.0, device=True)
on_device += [c.is_cuda for c in con]
for i, c in enumerate(con):
    out["con_%d" % i] = host(c)

first = sum(c.width * c.height for c in cams[:2])
image = depths[first:first + cams[2].width * cams[2].height]
pts = fi.depth_to_points(cams[2], image, 1.0)
on_device += [p.is_cuda for p in pts]
for i, p in enumerate(pts):
    out["pts_%d" % i] = host(p)
cmp_ = fi.depth_to_points(cams[2], image, 1.0, compact=True)
on_device += [p.is_cuda for p in cmp_]
for i, p in enumerate(cmp_[:3]):
    out["cmp_%d" % i] = host(p)

# add_volume against add_points of the device-resident constraints
f1, f2 = fi.LatticeField(sizes), fi.LatticeField(sizes)
for f in (f1, f2):
    f.add_field_constraints(fi.Weights())
f1.add_volume(again, 0.7, min_weight=1.0)
f2.add_points(0.7, fi.ValueKernel.kNearestNeighbor, 0.0, fi.GradientKernel.kNearestNeighbor, con[0], torch.zeros_like(con[0]), con[2], con[1])
out["diag_volume"], out["diag_points"] = f1.diag(), f2.diag()
out["on_device"] = np.array(on_device)
np.savez(dst, **out)
print("depth torch worker done")
