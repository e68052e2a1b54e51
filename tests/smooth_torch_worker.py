"""Worker of tests/test_gpu_smooth.py::test_device_pointers, started as a fresh process: torch brings its own HIP runtime and
must stay out of the pytest process.  The mesh and the field of <in.npz> go to the device as torch tensors, through
fi.smooth_mesh (with and without normals and keys), fi.mesh_normals and fi.iso_surface(largest=1, smooth=3); the answers come
back to <out.npz>."""
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
faired = fi.smooth_mesh(mesh, 4, boundary="slide", max_move=0.5)
on_device = [t.is_cuda for t in faired]
for k, v in zip(faired._fields, faired):
    out["taubin_" + k] = host(v)
bare = fi.smooth_mesh(mesh._replace(normals=None, keys=None), 2, mu=0.0)
out["bare_has_normals"] = np.array([0 if bare.normals is None else 1])
on_device += [bare.vertices.is_cuda, bare.indices.is_cuda, bare.keys.is_cuda]
for k in ("vertices", "indices", "keys"):
    out["bare_" + k] = host(getattr(bare, k))
made = fi.mesh_normals(mesh._replace(normals=None))
on_device += [t.is_cuda for t in made]
for k, v in zip(made._fields, made):
    out["normals_" + k] = host(v)
f = torch.from_numpy(a["f"]).cuda()
for k, v in zip(fi.IsoMesh._fields, fi.iso_surface(f, sizes, largest=1, smooth=3)):
    out["field_" + k] = v
out["on_device"] = np.array(on_device)
np.savez(dst, **out)
print("smooth torch worker done")
