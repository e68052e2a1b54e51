"""Worker of tests/test_gpu_meshpts.py::test_device_pointers, started as a fresh process: torch brings its own HIP runtime and
must stay out of the pytest process.  The two meshes of <in.npz> go to the device as torch tensors, through fi.sample_mesh
(with vertex normals and primitives; without normals and keys) and fi.mesh_deviation (symmetric, with vertex distances); the
answers come back to <out.npz>."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
a = np.load(src)
mesh = fi.IsoMesh(*[torch.from_numpy(a[k]).cuda() for k in fi.IsoMesh._fields])
other = fi.IsoMesh(torch.from_numpy(a["cube_vertices"]).cuda(), None, torch.from_numpy(a["cube_indices"]).cuda(), None)
host = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else x  # noqa: E731
out = {}
got = fi.sample_mesh(mesh, 5000, 3, normals="vertex", primitives=True)
on_device = [t.is_cuda for t in got]
for k, v in zip(("positions", "normals", "primitives"), got):
    out["sample_" + k] = host(v)
bare = fi.sample_mesh(mesh._replace(normals=None, keys=None), 777, 1, normals=None)
on_device.append(bare.is_cuda)
out["bare_positions"] = host(bare)
d = fi.mesh_deviation(mesh, other, 3000, 2, vertex_distances=True)
for side in ("a_to_b", "b_to_a"):
    for what in ("samples", "vertices"):
        for k, v in d[side][what].items():
            out["%s_%s_%s" % (side, what, k)] = np.asarray(v)
    on_device.append(d[side]["vertex_distances"].is_cuda)
    out[side + "_vertex_distances"] = host(d[side]["vertex_distances"])
out["on_device"] = np.array(on_device)
np.savez(dst, **out)
print("meshpts torch worker done")
