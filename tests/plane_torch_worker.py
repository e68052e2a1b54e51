"""Worker of tests/test_gpu_plane.py::test_device_tensors, started as a fresh process: torch brings its own HIP runtime and
must stay out of the pytest process.  The cloud and mask of <in.npz> go to the device as torch tensors, through segment_plane,
segment_planes and clean_points(remove_planes=...); the answers come back to <out.npz>."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
data = np.load(src)
pos = torch.from_numpy(data["pos"]).cuda()
mask = torch.from_numpy(data["mask"]).cuda()
host = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)  # noqa: E731

model, inliers = fi.segment_plane(pos, 0.15, mask=mask)
on_device = [inliers.is_cuda, inliers.dtype == torch.bool]
labels, models = fi.segment_planes(pos, 0.15, 2, min_inliers=500)
on_device += [labels.is_cuda, labels.dtype == torch.int32]
cleaned, _, _, report = fi.clean_points(pos, remove_planes=dict(threshold=0.15, max_planes=2, min_inliers=500))
on_device += [cleaned.is_cuda, report["output"] == len(cleaned), report["planes"] == models[0]["inliers"]]
np.savez(dst, inliers=host(inliers), ints=np.array([int(model[k]) for k in ("found", "refits", "inliers", "candidates", "trials")]),
         doubles=np.array(list(model["normal"]) + [model["offset"], model["rms"]]), labels=host(labels), planes=len(models),
         clean_pos=host(cleaned), on_device=np.array(on_device))
print("plane torch worker done")
