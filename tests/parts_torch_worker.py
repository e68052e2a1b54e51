"""Worker of tests/test_gpu_mesh_parts.py::test_device_pointers, started as a fresh process: torch brings its own HIP runtime
and must stay out of the pytest process.  The mesh and the field of <in.npz> go to the device as torch tensors, through
fi.mesh_parts, fi.select_parts and fi.iso_surface(parts=True / largest=1); the answers come back to <out.npz>."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
a = np.load(src)
sizes = [int(s) for s in a["sizes"]]
mesh = fi.IsoMesh(*[torch.from_numpy(a[k]).cuda() for k in fi.IsoMesh._fields])
host = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else x  # noqa: E731
out = {}
parts = fi.mesh_parts(mesh)
out["labels_on_device"] = np.array([parts.vertex_labels.is_cuda and parts.primitive_labels.is_cuda])
for k, v in zip(parts._fields, parts):
    out["parts_" + k] = host(v)
selected = fi.select_parts(mesh, a["keep"])
out["selection_on_device"] = np.array([all(t.is_cuda for t in selected)])
for k, v in zip(selected._fields, selected):
    out["selected_" + k] = host(v)
f = torch.from_numpy(a["f"]).cuda()
_whole, field_parts = fi.iso_surface(f, sizes, parts=True)
for k, v in zip(field_parts._fields, field_parts):
    out["field_parts_" + k] = host(v)
for k, v in zip(fi.IsoMesh._fields, fi.iso_surface(f, sizes, largest=1)):
    out["largest_" + k] = v
np.savez(dst, **out)
print("parts torch worker done")
