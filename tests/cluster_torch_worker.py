"""Worker of tests/test_gpu_cluster.py::test_device_tensors, started as a fresh process: torch brings its own HIP runtime and
must stay out of the pytest process.  The cloud of <in.npz> goes to the device as a torch tensor, through PointIndex.cluster and
LatticeField.cluster, cluster_measure, cluster_points and clean_points; the answers come back to <out.npz>."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
pos = torch.from_numpy(np.load(src)["pos"]).cuda()
host = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)  # noqa: E731
out, on_device = {}, []

field = fi.LatticeField([32, 32, 32])
field.add_field_constraints(fi.Weights())
field.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 0.0, fi.GradientKernel.kCellEdges, pos)
for name, index in (("pts", fi.PointIndex(pos)), ("ctx", field)):
    labels, core, stats = index.cluster(0.6, 4, core=True, stats=True, device=True)
    on_device += [labels.is_cuda, core.is_cuda, labels.dtype == torch.int32, core.dtype == torch.bool]
    out.update({name + "_labels": host(labels), name + "_core": host(core),
                name + "_stats": np.array([stats[k] for k in ("clusters", "core", "border", "noise", "non_finite")])})

rows = fi.cluster_measure(pos, labels, core)            # device tensors in, the rows on the host
out.update(count=np.array([r["count"] for r in rows]), cores=np.array([r["core"] for r in rows]),
           lo=np.stack([r["lo"] for r in rows]), hi=np.stack([r["hi"] for r in rows]), centroid=np.stack([r["centroid"] for r in rows]))
only = fi.cluster_points(pos, 1.5)
cleaned, _, _, report = fi.clean_points(pos, cluster_eps=1.5, largest=1)
on_device += [only.is_cuda, cleaned.is_cuda, report["output"] == len(cleaned), report["cluster"] == 30]
out.update(labels_only=host(only), clean_pos=host(cleaned), on_device=np.array(on_device))
np.savez(dst, **out)
print("cluster torch worker done")
