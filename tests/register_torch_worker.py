"""Worker of tests/test_gpu_register.py::test_device_pointers, started as a fresh process: torch brings its own HIP runtime and
must stay out of the pytest process.  The cube, its sample points and the source of <in.npz> go to the device as torch tensors,
through fi.register_points against the mesh, against the points with normals and against the bare points; the answers come
back to <out.npz>."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
a = np.load(src)
dev = {k: torch.from_numpy(a[k]).cuda() for k in a.files}
mesh = fi.IsoMesh(dev["vertices"], None, dev["indices"], None)
host = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)  # noqa: E731
out, on_device = {}, []
runs = {"mesh": fi.register_points(dev["source"], mesh, max_iterations=4, transformed=True, distances=True),
        "set": fi.register_points(dev["source"], dev["points"], dev["normals"], max_iterations=4, transformed=True, distances=True),
        "point": fi.register_points(dev["source"], dev["points"], mode="point", max_iterations=2, transformed=True, distances=True)}
for name, r in runs.items():
    on_device += [r["transformed"].is_cuda, r["distances"].is_cuda]
    for k, v in r.items():
        out["%s_%s" % (name, k)] = host(v)
moved = fi.apply_transform(runs["mesh"]["transform"], dev["source"])
on_device.append(moved.is_cuda and moved.dtype == torch.float64)
out["on_device"] = np.array(on_device)
np.savez(dst, **out)
print("register torch worker done")
