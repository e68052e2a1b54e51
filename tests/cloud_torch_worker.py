"""Worker of tests/test_gpu_cloud.py::test_device_tensors, started as a fresh process: torch brings its own HIP runtime and
must stay out of the pytest process.  The cloud, its normals, values and queries of <in.npz> go to the device as torch tensors,
through the four PointIndex / LatticeField entries, thin_points and clean_points; the answers come back to <out.npz>."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
a = np.load(src)
dev = {k: torch.from_numpy(a[k]).cuda() for k in a.files}
host = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)  # noqa: E731
out, on_device = {}, []

field = fi.LatticeField([32, 32, 32])
field.add_field_constraints(fi.Weights())
field.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, dev["pos"])
for name, index in (("pts", fi.PointIndex(dev["pos"])), ("ctx", field)):
    count = index.radius_count(dev["q"], 1.5, 6)
    mean, kth, m = index.neighbour_distances(12, device=True)
    stat_keep, stats = index.statistical_outliers(12, 1.0, device=True)
    radius_keep, kept = index.radius_outliers(1.5, 2, device=True)
    on_device += [t.is_cuda for t in (count, mean, kth, m, stat_keep, radius_keep)]
    on_device.append(kept == int(radius_keep.sum()) and stats["kept"] == int(stat_keep.sum()))
    out.update({name + "_count": host(count), name + "_mean": host(mean), name + "_kth": host(kth), name + "_m": host(m),
                name + "_stat_keep": host(stat_keep), name + "_radius_keep": host(radius_keep),
                name + "_stats": np.array([stats["counted"], stats["kept"], stats["mean"], stats["stddev"], stats["threshold"]])})

thin = fi.thin_points(dev["pos"], 0.75, dev["nrm"], dev["val"], [0.1, 0.2, 0.3], "mean", counts=True, indices=True, cell_map=True)
on_device += [t.is_cuda for t in thin]
for key, t in zip(("positions", "normals", "values", "counts", "indices", "cell_map"), thin):
    out["thin_" + key] = host(t)
pos, nrm, val, report = fi.clean_points(dev["pos"], dev["nrm"], dev["val"], cell=0.5, radius=1.5, k=8, std_ratio=1.0)
on_device += [pos.is_cuda, nrm.is_cuda, val.is_cuda, report["output"] == len(pos)]
out.update(clean_pos=host(pos), clean_nrm=host(nrm), clean_val=host(val))
out["on_device"] = np.array(on_device)
np.savez(dst, **out)
print("cloud torch worker done")
