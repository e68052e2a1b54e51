"""Times the images of a lattice field on the device (fi_march.hip) beside the mesh renderer's image of the same field's
iso-surface (fi_ray.hip), in one run: the 512^3 analytic sphere of tools/ray_time.py, a 1024^2 pinhole image from that tool's
viewpoint (profiles/march.md holds the numbers).

    python tools/march_time.py [side]             default 512
    python tools/march_time.py summarize <kernel_trace.csv>     (of a run under rocprofv3 --kernel-trace --stats)

The field, the volume's arrays and the mesh path's rays live on the device (torch tensors), so a call moves no field and no
image across the bus; every entry point ends with a stream synchronise, so the host clock around a call is the call's time.
The phases, each run once to warm up and then REPS windows of CALLS back-to-back calls, in this order:
  field 1      render_field, step 1, refine 4                                  k_march_image<false>
  field 0.5    render_field, step 0.5, refine 4                                k_march_image<false>
  field all    render_field, step 1, with positions, normals and incidences    k_march_image<false>
  volume 1     DepthVolume.render of the same values under unit weights        k_march_image<true>
  mesh rays    SurfaceIndex.raycast of the same pixels' rays (what             k_ray_hit<3>
               SurfaceIndex.render_depth launches, without its host-side ray set-up)
and once each, as they are one-off costs of the mesh path: iso_surface of the field and the surface tree's build.
"""
import csv
import math
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5
CALLS = 5
IMAGE = 1024
BOOL = {"false": r"(false|\(bool\)0)", "true": r"(true|\(bool\)1)"}
# (phase, the kernel it launches once per call)
PHASES = [("field, step 1", r"k_march_image<%s>" % BOOL["false"]), ("field, step 0.5", r"k_march_image<%s>" % BOOL["false"]),
          ("field, step 1, every output", r"k_march_image<%s>" % BOOL["false"]), ("volume, step 1", r"k_march_image<%s>" % BOOL["true"]),
          ("mesh rays", r"k_ray_hit<3>")]


def timed(what, call):
    out = call()  # warm-up (allocations, code objects)
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            out = call()
        ts.append(1e3 * (time.perf_counter() - t0) / CALLS)
    print("%s: %.3f ms per call (median of %d windows of %d calls, [%.3f, %.3f], host wall)" % (what, np.median(ts), REPS, CALLS, min(ts), max(ts)))
    return out


def run(n):
    import torch

    import field_interpolation_amd as fi
    c, r = (n - 1) / 2.0 + 0.3, 0.35 * n
    ax = torch.arange(n, dtype=torch.float32, device="cuda")
    f = torch.sqrt((ax[None, None, :] - c) ** 2 + (ax[None, :, None] - c) ** 2 + (ax[:, None, None] - c) ** 2).sub_(r).reshape(-1)
    sizes = [n, n, n]
    eye, centre = [1.6 * n, -0.9 * n, 1.1 * n], [c, c, c]
    cam = fi.camera_look_at(eye, centre, [0, 0, 1], 0.6, IMAGE, IMAGE)
    print("sphere %d^3, radius %.1f, image %d^2" % (n, r, IMAGE))
    depth = timed("field, step 1", lambda: fi.render_field(f, sizes, cam))
    half = timed("field, step 0.5", lambda: fi.render_field(f, sizes, cam, step=0.5))
    timed("field, step 1, every output", lambda: fi.render_field(f, sizes, cam, positions=True, normals=True, incidence=True))
    vol = fi.DepthVolume(sizes, 3.0).load(f, torch.ones_like(f))
    dvol = timed("volume, step 1", lambda: vol.render(cam, device=True))
    print("  %d of %d pixels hit (step 0.5: %d, volume: %d)" % (torch.isfinite(depth).sum(), depth.numel(), torch.isfinite(half).sum(), torch.isfinite(dvol).sum()))
    t0 = time.perf_counter()
    mesh = fi.iso_surface(f, sizes, normals=False)
    t1 = time.perf_counter()
    s = fi.SurfaceIndex.from_mesh(mesh)
    t2 = time.perf_counter()
    print("mesh path, once: iso_surface %.1f ms (with its copy to the host), surface tree %.1f ms, %d triangles" % (1e3 * (t1 - t0), 1e3 * (t2 - t1), s.num_primitives))
    # SurfaceIndex.render_depth's rays, on the device
    fwd = np.array(centre) - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0, 0, 1])
    right /= np.linalg.norm(right)
    top = np.cross(right, fwd)
    px = ((np.arange(IMAGE) + 0.5) / IMAGE * 2 - 1) * math.tan(0.3)
    dd = fwd + px[None, :, None] * right - px[:, None, None] * top
    dd /= np.linalg.norm(dd, axis=2, keepdims=True)
    dd = torch.from_numpy(dd.reshape(-1, 3).astype(np.float32)).cuda()
    oo = torch.from_numpy(np.broadcast_to(np.array(eye, np.float32), dd.shape).copy()).cuda()
    tm, _prim = timed("mesh rays", lambda: s.raycast(oo, dd))
    both = torch.isfinite(tm) & torch.isfinite(depth.reshape(-1))
    print("  %d of %d rays hit the mesh; |field depth - mesh depth| over the %d pixels both hit: mean %.4f, max %.4f"
          % (torch.isfinite(tm).sum(), tm.numel(), both.sum(), (tm - depth.reshape(-1))[both].abs().mean(), (tm - depth.reshape(-1))[both].abs().max()))
    t0 = time.perf_counter()
    s.render_depth(eye, centre, [0, 0, 1], 0.6, IMAGE, IMAGE)
    print("SurfaceIndex.render_depth as it stands (rays set up on the host, arrays copied): %.1f ms" % (1e3 * (time.perf_counter() - t0)))


def summarize(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    taken = {}
    per = 1 + REPS * CALLS
    print("| phase | kernel | kernel time, ms (median of %d) |" % (REPS * CALLS))
    print("|---|---|---:|")
    for phase, pattern in PHASES:
        runs = [e - s for s, e, k in rows if re.search(pattern, k)]
        first = taken.get(pattern, 0)
        mine = runs[first: first + per]
        taken[pattern] = first + per
        assert len(mine) == per, (phase, len(runs))
        print("| %s | `%s` | %.3f |" % (phase, pattern.split("<")[0], np.median(mine[1:]) * 1e-6))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "summarize":
        summarize(sys.argv[2])
        sys.exit(0)
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
