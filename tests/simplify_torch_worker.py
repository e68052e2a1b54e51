"""Worker of tests/test_gpu_simplify.py::test_device_pointers, started as a fresh process: torch brings its own HIP runtime and
must stay out of the pytest process.  The mesh and the field of <in.npz> go to the device as torch tensors, through
fi.simplify_mesh (with and without normals and keys) and fi.iso_surface(largest=1, simplify=2.0); the answers come back to
<out.npz>."""
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
coarse, vmap = fi.simplify_mesh(mesh, 2.0, origin=(-0.37, 0.21, 0.5), vertex_map=True)
on_device = [t.is_cuda for t in coarse] + [vmap.is_cuda]
for k, v in zip(coarse._fields, coarse):
    out["quadric_" + k] = host(v)
out["quadric_map"] = host(vmap)
bare = fi.simplify_mesh(mesh._replace(normals=None, keys=None), 3.0, placement="mean")
out["mean_has_normals"] = np.array([0 if bare.normals is None else 1])
on_device += [bare.vertices.is_cuda, bare.indices.is_cuda, bare.keys.is_cuda]
for k in ("vertices", "indices", "keys"):
    out["mean_" + k] = host(getattr(bare, k))
f = torch.from_numpy(a["f"]).cuda()
for k, v in zip(fi.IsoMesh._fields, fi.iso_surface(f, sizes, largest=1, simplify=2.0)):
    out["field_" + k] = v
out["on_device"] = np.array(on_device)
np.savez(dst, **out)
print("simplify torch worker done")
