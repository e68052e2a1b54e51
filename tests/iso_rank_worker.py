#!/usr/bin/env python3
"""Worker of tests/test_gpu_iso_slabs.py, started by torch.distributed.run with two ranks on ONE GPU: each rank solves its
slab of a 3-D SDF problem through the host-staged test transport (fi_comm_init_host), then extracts its piece of the
iso-surface from its solution in place (ghost planes exchanged by fi_iso_extract) and from its owned values passed in.
Rank 0 writes every rank's owned solution and pieces to FI_ISO_OUT (.npz) for the test to merge and compare."""
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

torch.cuda.set_device(0)

sizes = [28, 26, 24]
pos, nrm = sphere_points(np.random.default_rng(3), sizes, 3000)
f = fi.LatticeField(sizes, rank=rank, nranks=world)
fdist.init_comm(f, None, host_staged=True)
f.add_field_constraints(fi.Weights())
zlo, zhi = f.point_range()
keep = (pos[:, 2] >= zlo) & (pos[:, 2] < zhi)
f.add_points(1.0, fi.ValueKernel.kLinearInterpolation, 1.0, fi.GradientKernel.kCellEdges, pos[keep], nrm[keep], None)
f.assemble()
x, it, rel = f.solve_cg(None, 0, 1e-6)
a = f.iso_surface()
b = f.iso_surface(x)
parts = [None] * world
dist.gather_object((x, tuple(a), tuple(b)), parts if rank == 0 else None, dst=0)
if rank == 0:
    out = {"sizes": np.array(sizes)}
    for r, (xr, ar, br) in enumerate(parts):
        out["x%d" % r] = xr
        for tag, m in (("a", ar), ("b", br)):
            for name, arr in zip(("vertices", "normals", "indices", "keys"), m):
                out["%s%d_%s" % (tag, r, name)] = arr
    np.savez(os.environ["FI_ISO_OUT"], **out)
del f
dist.barrier()
print("DONE rank %d" % rank)
