"""Worker of tests/test_gpu_dual.py::test_memory_kinds_and_iso, started as a fresh process: torch brings its own HIP runtime
and must stay out of the pytest process.  The field and gradients of <in.npz> go to the device as torch tensors, through
fi.dual_contour and LatticeField.dual_contour; the meshes come back to <out.npz>."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
a = np.load(src)
sizes = [int(s) for s in a["sizes"]]
iso = float(a["iso"])
f = torch.from_numpy(a["f"]).cuda()
g = torch.from_numpy(a["g"]).cuda()
out = {}
for name, mesh in (("plain", fi.dual_contour(f, sizes, iso)), ("grad", fi.dual_contour(f, sizes, iso, g)),
                   ("ctx", fi.LatticeField(sizes).dual_contour(f, iso, g))):
    for k, v in zip(("vertices", "normals", "indices", "keys"), mesh):
        out[name + "_" + k] = v
try:
    fi.dual_contour(a["f"], sizes, iso, g)
    out["mixed_refused"] = np.array([False])
except ValueError:
    out["mixed_refused"] = np.array([True])
np.savez(dst, **out)
print("dual torch worker done")
