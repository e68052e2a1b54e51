"""Times the normal orientation (fi_orient.hip) on the device next to the normal estimation on the same points
(profiles/orient.md holds the numbers).  Points, normals and outputs live on the device (torch tensors).

    python tools/orient_time.py config4 [side]   config 4's 1 M points uniformly random in its 256^3 lattice
    python tools/orient_time.py config5 [side]   config 5's 5 M points on a sphere in its 512^3 lattice

The library itself reports each call's parts with FI_ORIENT_STATS set (device events around the neighbour table and around
everything after it, the Boruvka rounds, the launches per round): one line per call on stderr, the first being the warm-up.
Run it under rocprofv3 --kernel-trace --stats, in a run of its own, for the per-kernel times.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

os.environ["FI_ORIENT_STATS"] = "1"
REPS = 5


def wall(label, fn):
    import torch
    fn()  # warm-up
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    print("%-40s median %10.3f ms, min %10.3f ms per call (wall, %d calls)" % (label, np.median(t), np.min(t), REPS), flush=True)


def main(kind, side):
    import torch

    import field_interpolation_amd as fi
    from normals_time import points
    sizes, pos = points(kind, side)
    print("%s: %d points, lattice %s" % (kind, len(pos), "x".join(map(str, sizes))), flush=True)
    pd = torch.from_numpy(pos).cuda()
    idx = fi.PointIndex(pd)
    wall("estimate_normals k = 16", lambda: idx.estimate_normals(k=16, device=True))
    nrm = idx.estimate_normals(k=16, device=True)
    wall("orient_normals k = 16, no guide", lambda: idx.orient_normals(nrm, k=16, components=True))
    view = torch.tensor([[-10.0 * sizes[0], 0.5 * sizes[1], 0.5 * sizes[2]]], dtype=torch.float32, device="cuda")
    wall("orient_normals k = 16, one viewpoint", lambda: idx.orient_normals(nrm, k=16, viewpoints=view, components=True))
    out, comp = idx.orient_normals(nrm, k=16, components=True)
    live = comp >= 0
    print("components: %d; live points: %d" % (int(torch.unique(comp[live]).numel()), int(live.sum())))
    if kind == "config5":
        c = torch.tensor([0.5 * (s - 1) for s in sizes], dtype=torch.float32, device="cuda")
        print("outward: %.4f propagated, %.4f canonical" % (float(((out * (pd - c)).sum(1) > 0).float().mean()),
                                                             float(((nrm * (pd - c)).sum(1) > 0).float().mean())))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "config4", int(sys.argv[2]) if len(sys.argv) > 2 else 0)
