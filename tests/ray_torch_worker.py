"""Worker of tests/test_gpu_ray.py::test_device_tensors, started as a fresh process: torch brings its own HIP runtime and
must stay out of the pytest process.  The mesh and rays of <in.npz> go to the device as torch tensors; the results of
every ray call of SurfaceIndex come back to <out.npz>, with flags for where each output lived."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
a = np.load(src)
sizes = [int(s) for s in a["sizes"]]
s = fi.SurfaceIndex(torch.from_numpy(a["v"]).cuda(), torch.from_numpy(a["i"]).cuda())
o, d = torch.from_numpy(a["o"]).cuda(), torch.from_numpy(a["d"]).cuda()
out, on = {}, []
t, j, b = s.raycast(o, d, 0.5, 40.0, bary=True)
on.append(t.is_cuda and j.is_cuda and b.is_cuda and j.dtype == torch.int64)
out["t"], out["j"], out["b"] = t.cpu().numpy(), j.cpu().numpy(), b.cpu().numpy()
c = s.count_hits(o, d, 0.5, 40.0, limit=2)
on.append(c.is_cuda and c.dtype == torch.int32)
out["c"] = c.cpu().numpy()
inside = s.contains(o, [0, 1, 1])
on.append(inside.is_cuda and inside.dtype == torch.bool)
out["inside"] = inside.cpu().numpy()
sd, sp, sc = s.signed_distance(o, 6.0, primitives=True, closest=True)
on.append(sd.is_cuda and sp.is_cuda and sc.is_cuda)
out["sd"], out["sp"], out["sc"] = sd.cpu().numpy(), sp.cpu().numpy(), sc.cpu().numpy()
sf, sfp = s.signed_distance_field(sizes, primitives=True, device=True)
on.append(sf.is_cuda and sfp.is_cuda)
out["sf"], out["sfp"] = sf.cpu().numpy(), sfp.cpu().numpy()
out["sdf"] = fi.mesh_to_sdf(fi.IsoMesh(a["v"], None, a["i"], None), sizes)
e = s.raycast(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), device="cuda"), bary=True)
ec = s.count_hits(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), device="cuda"))
out["empty_ok"] = np.array([e[0].shape == (0,) and e[1].shape == (0,) and tuple(e[2].shape) == (0, 2) and e[0].is_cuda
                            and ec.shape == (0,)])
out["on_device"] = np.array(on)
np.savez(dst, **out)
print("ray torch worker done")
