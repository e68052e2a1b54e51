"""Times the ray queries on the device (fi_ray.hip) against the mesh of an analytic sphere's exact signed distance (the
512^3 sphere of profiles/redistance.md); run it under rocprofv3 --kernel-trace --stats for the per-kernel times
(profiles/raycast.md holds the numbers).

    python tools/ray_time.py [side]               default 512
    python tools/ray_time.py summarize <kernel_trace.csv>

The phases, each run once to warm up and REPS times timed, in this order:
  pinhole    a 1024^2 depth image (SurfaceIndex.render_depth)                              k_ray_hit<3>
  ortho      1024^2 parallel rays along +y from a plane in front of the lattice            k_ray_hit<3>
  near 4     SurfaceIndex.distance of 1024^2 points of the plane z = centre, max_distance 4   k_surf_query<3, 0>
  near inf   the same, unbounded                                                           k_surf_query<3, 0>
  shadow     count_hits with limit 1 of the pinhole rays (is anything in the way)          k_ray_count<3, 0>
  signed     signed_distance_field at 256^3, max_distance 4: the distance pass              k_surf_query<3, 1>
             and the sign pass that follows it                                             k_ray_count<3, 3>
`summarize` takes the launches of each kernel in order and prints the medians of the timed ones.
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

REPS = 3
IMAGE = 1024
FIELD = 256
# (phase, the kernel it launches once per call)
PHASES = [("pinhole", r"k_ray_hit<3>"), ("ortho", r"k_ray_hit<3>"), ("near 4", r"k_surf_query<3,\s*0>"),
          ("near inf", r"k_surf_query<3,\s*0>"), ("shadow", r"k_ray_count<3,\s*0>"), ("signed: distance pass", r"k_surf_query<3,\s*1>"),
          ("signed: sign pass", r"k_ray_count<3,\s*3>")]


def timed(what, call):
    out = call()  # warm-up (allocations, code objects)
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = call()
        ts.append(1e3 * (time.perf_counter() - t0))
    print("%s: %.1f ms per call (median of %d, host wall, copies included)" % (what, np.median(ts), REPS))
    return out


def run(n):
    import field_interpolation_amd as fi
    c, r = (n - 1) / 2.0 + 0.3, 0.35 * n
    ax = np.arange(n, dtype=np.float32)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    f = (np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - r).astype(np.float32).reshape(-1)
    del x, y, z
    mesh = fi.iso_surface(f, [n, n, n], normals=False)
    del f
    s = fi.SurfaceIndex.from_mesh(mesh)
    print("sphere %d^3, radius %.1f: %d triangles" % (n, r, s.num_primitives))
    eye, centre = [1.6 * n, -0.9 * n, 1.1 * n], [c, c, c]
    t, _p = timed("pinhole %d^2" % IMAGE, lambda: s.render_depth(eye, centre, [0, 0, 1], 0.6, IMAGE, IMAGE))
    print("  %d of %d pixels hit" % (np.isfinite(t).sum(), t.size))
    u = np.linspace(0, n - 1, IMAGE, dtype=np.float32)
    gx, gz = np.meshgrid(u, u)
    o = np.stack([gx.ravel(), np.full(gx.size, -10, np.float32), gz.ravel()], 1)
    d = np.broadcast_to(np.array([0, 1, 0], np.float32), o.shape)
    t, _p = timed("ortho %d^2" % IMAGE, lambda: s.raycast(o, d))
    print("  %d of %d rays hit" % (np.isfinite(t).sum(), t.size))
    q = np.stack([gx.ravel(), gz.ravel(), np.full(gx.size, round(c), np.float32)], 1)
    for md in (4.0, math.inf):
        dist = timed("nearest triangle of %d^2 points, max_distance %g" % (IMAGE, md), lambda: s.distance(q, md))
        print("  %d of %d finite" % (np.isfinite(dist).sum(), dist.size))
    # the pinhole rays again, as shadow rays
    fwd = np.array(centre) - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0, 0, 1])
    right /= np.linalg.norm(right)
    top = np.cross(right, fwd)
    px = ((np.arange(IMAGE) + 0.5) / IMAGE * 2 - 1) * math.tan(0.3)
    dd = (fwd + px[None, :, None] * right - px[:, None, None] * top).reshape(-1, 3).astype(np.float32)
    oo = np.broadcast_to(np.array(eye, np.float32), dd.shape)
    cnt = timed("shadow rays %d^2 (limit 1)" % IMAGE, lambda: s.count_hits(oo, dd, limit=1))
    print("  %d of %d blocked" % (cnt.sum(), cnt.size))
    sd = timed("signed_distance_field %d^3, max_distance 4" % FIELD, lambda: s.signed_distance_field([FIELD] * 3, 4.0))
    print("  %d of %d finite, %d inside" % (np.isfinite(sd).sum(), sd.size, np.signbit(sd).sum()))


def summarize(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    taken = {}
    print("| phase | kernel | kernel time, ms (median of %d) |" % REPS)
    print("|---|---|---:|")
    for phase, pattern in PHASES:
        runs = [e - s for s, e, k in rows if re.search(pattern, k)]
        first = taken.get(pattern, 0)
        mine = runs[first: first + 1 + REPS]
        taken[pattern] = first + 1 + REPS
        assert len(mine) == 1 + REPS, (phase, len(runs))
        print("| %s | `%s` | %.3f |" % (phase, pattern.replace(r"\s*", " "), np.median(mine[1:]) * 1e-6))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "summarize":
        summarize(sys.argv[2])
        sys.exit(0)
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
