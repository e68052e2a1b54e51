"""Worker of tests/test_gpu_shape.py::test_device_tensors, started as a fresh process: torch brings its own HIP runtime and
must stay out of the pytest process.  The cloud, normals and mask of <in.npz> go to the device as torch tensors, through
segment_cylinder, segment_sphere and segment_shapes; the answers come back to <out.npz>."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
data = np.load(src)
pos = torch.from_numpy(data["pos"]).cuda()
nrm = torch.from_numpy(data["nrm"]).cuda()
mask = torch.from_numpy(data["mask"]).cuda()
host = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)  # noqa: E731
INTS = ("found", "refits", "inliers", "candidates", "trials")

cyl, cyl_inliers = fi.segment_cylinder(pos, nrm, 0.05, 0.1, 2.0, mask=mask)
on_device = [cyl_inliers.is_cuda, cyl_inliers.dtype == torch.bool]
sph, sph_inliers = fi.segment_sphere(pos, 0.05, 0.5, 5.0, normals=nrm, max_angle=20.0)
on_device += [sph_inliers.is_cuda, sph_inliers.dtype == torch.bool]
labels, models = fi.segment_shapes(pos, "cylinder", 0.05, 2, min_inliers=500, normals=nrm, r_min=0.1, r_max=2.0)
on_device += [labels.is_cuda, labels.dtype == torch.int32]
mixed = False
try:
    fi.segment_cylinder(pos, data["nrm"], 0.05)          # positions on the device, normals on the host
except ValueError:
    mixed = True
on_device.append(mixed)
np.savez(dst, cyl_inliers=host(cyl_inliers), cyl_ints=np.array([int(cyl[k]) for k in INTS]),
         cyl_doubles=np.array(list(cyl["center"]) + [cyl["radius"], cyl["rms"]] + list(cyl["axis"]) + list(cyl["extent"])),
         sph_inliers=host(sph_inliers), sph_ints=np.array([int(sph[k]) for k in INTS]),
         sph_doubles=np.array(list(sph["center"]) + [sph["radius"], sph["rms"]]), labels=host(labels), shapes=len(models),
         on_device=np.array(on_device))
print("shape torch worker done")
