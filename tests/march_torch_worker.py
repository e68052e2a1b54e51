"""Worker of tests/test_gpu_march.py::test_device_tensors, started as a fresh process: torch brings its own HIP runtime and
must stay out of the pytest process.  The field, weight and rays of <in.npz> go to the device as torch tensors, through
raycast_field, render_field, DepthVolume.render and DepthVolume.track; the answers come back to <out.npz>."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
a = np.load(src)
dev = lambda k: torch.from_numpy(a[k]).cuda()  # noqa: E731
host = lambda x: x.cpu().numpy()  # noqa: E731
out, on_device = {}, []
sizes = [int(s) for s in a["sizes"]]
shape = a["shape"]
cam = fi.Camera(a["pose"], *a["intr"], int(shape[0]), int(shape[1]), "z" if shape[2] == 0 else "range")

field, weight = dev("field"), dev("weight")
rays = fi.raycast_field(field, sizes, dev("o"), dev("d"), side="either", weight=weight, min_weight=0.5, positions=True, normals=True)
on_device += [x.is_cuda for x in rays]
for name, x in zip(("t", "side", "positions", "normals"), rays):
    out["ray_" + name] = host(x)

image = fi.render_field(field, sizes, cam, weight=weight, min_weight=0.5, positions=True, normals=True, incidence=True)
on_device += [x.is_cuda for x in image]
for name, x in zip(("depth", "positions", "normals", "incidence"), image):
    out["img_" + name] = host(x)

vol = fi.DepthVolume([32, 32, 32], 3.0, 64.0).load(dev("tsdf"), dev("wt"))
guess = fi.Camera(a["guess"], *a["gintr"], 48, 48, "range")
image = vol.render(guess, positions=True, normals=True, incidence=True, device=True)
on_device += [x.is_cuda for x in image]
for name, x in zip(("depth", "positions", "normals", "incidence"), image):
    out["vol_" + name] = host(x)

tracked, info = vol.track(guess, dev("depth").reshape(48, 48), rounds=2)
out["track_pose"], out["track_correction"] = tracked.pose, info["correction"]
out["on_device"] = np.array(on_device)
np.savez(dst, **out)
print("march torch worker done")
