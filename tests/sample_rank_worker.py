#!/usr/bin/env python3
"""Worker of tests/test_gpu_sample_slabs.py, started by torch.distributed.run with two ranks on ONE GPU: each rank solves its
slab of a 3-D SDF problem through the host-staged test transport (fi_comm_init_host), then samples the field at the same
points as the other rank -- its solution in place (ghost planes exchanged by fi_sample) and its owned values passed in,
linear and cubic with gradients.  Rank 0 writes every rank's owned solution and results to FI_SAMPLE_OUT (.npz)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch
import torch.distributed as dist

dist.init_process_group("gloo")     # before any GPU call
rank, world = dist.get_rank(), dist.get_world_size()

import field_interpolation_amd as fi                      # noqa: E402
from field_interpolation_amd import dist as fdist         # noqa: E402
from util import sphere_points                            # noqa: E402
from test_gpu_sample_slabs import seam_points             # noqa: E402

torch.cuda.set_device(0)

sizes = [28, 26, 24]
pts, nrm = sphere_points(np.random.default_rng(3), sizes, 3000)
pos = np.concatenate([seam_points(np.random.default_rng(4), sizes, world), pts])   # the same points on every rank
f = fi.LatticeField(sizes, rank=rank, nranks=world)
fdist.init_comm(f, None, host_staged=True)
f.add_field_constraints(fi.Weights())
zlo, zhi = f.point_range()
keep = (pts[:, 2] >= zlo) & (pts[:, 2] < zhi)
f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 1.0, fi.GradientKernel.kCellEdges, pts[keep], nrm[keep], None)
f.assemble()
x, it, rel = f.solve_cg(None, 0, 1e-6)
res = {}
for cubic in (0, 1):
    res["a_v%d" % cubic], res["a_g%d" % cubic] = f.sample(pos, gradients=True, cubic=bool(cubic))
    res["b_v%d" % cubic], res["b_g%d" % cubic] = f.sample(pos, x, gradients=True, cubic=bool(cubic))
parts = [None] * world
dist.gather_object((x, res), parts if rank == 0 else None, dst=0)
if rank == 0:
    out = {"sizes": np.array(sizes), "pos": pos}
    for r, (xr, rr) in enumerate(parts):
        out["x%d" % r] = xr
        for k, v in rr.items():
            tag, name = k.split("_")
            out["%s%d_%s" % (tag, r, name)] = v
    np.savez(os.environ["FI_SAMPLE_OUT"], **out)
del f
dist.barrier()
print("DONE rank %d" % rank)
