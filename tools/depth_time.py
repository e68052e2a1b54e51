"""Times the depth unit (fi_depth.hip) on the device next to its yardstick (profiles/depth.md is where the numbers go):
DepthVolume.integrate of m = 1, 4, 16 range images of 640 x 480 into a side^3 volume (default 256), with and without the
wave-uniform cull (FI_NO_DEPTH_CULL), and of 16 images handed over c = 1, 2, 4, 8 at a call -- what a launch of c cameras
costs, the question FI_DEPTH_CAMERAS answers -- beside a plain device copy of the bytes one pass over the volume moves (tsdf
and weight read and written: 16 B a voxel).  Two sets of views of a sphere: "wide" cameras see the whole lattice, "narrow"
ones about a sixth of it, which is where a cull can pay.  depth_to_points of one image and constraints() are timed as well.

    python tools/depth_time.py [side]

Inputs are device tensors.  Every call is made once as a warm-up; a window is INNER calls back to back between two HIP events
on the stream the library works on (a single call lasts a fraction of a millisecond: too short a window by itself), and the
figure is the median over REPS windows of the time per call, with the fastest and the slowest window beside it.  A call
includes what the library does on the host: staging the camera table and the stream synchronise every entry point ends with.
Nothing outside the tree is read."""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 9
INNER = 20
WIDTH, HEIGHT = 640, 480


def timed(label, fn, per=1):
    import torch
    fn()  # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / (per * INNER))
    print("%-74s median of %d x %d: %8.3f ms (min %.3f, max %.3f)" % (label, REPS, INNER, statistics.median(ms), min(ms), max(ms)))
    return out


def views(fi, side, fov, count=16):
    """count cameras around a sphere of radius 0.3 side in the middle of the lattice, and its range images"""
    import numpy as np
    centre = np.full(3, 0.5 * (side - 1))
    rng = np.random.default_rng(2)
    cams, depths = [], []
    for _ in range(count):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        eye = centre + 1.3 * side * d
        cam = fi.camera_look_at(eye, centre + 0.2 * side * rng.normal(size=3) * (fov < 0.5), np.cross(d, rng.normal(size=3)), fov, WIDTH, HEIGHT)
        R, t = cam.pose[:, :3].astype(np.float64), cam.pose[:, 3].astype(np.float64)
        rows, cols = np.meshgrid(np.arange(HEIGHT), np.arange(WIDTH), indexing="ij")
        ray = np.stack([(cols + 0.5 - cam.cx) / cam.fx, (rows + 0.5 - cam.cy) / cam.fy, np.ones(rows.shape)], axis=-1)
        ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
        ray = ray @ R
        oc = -R.T @ t - centre
        b = ray @ oc
        disc = b * b - (oc @ oc - (0.3 * side) ** 2)
        hit = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), np.inf)
        cams.append(cam)
        depths.append(hit.astype(np.float32))
    return cams, depths


def main(side):
    import torch

    import field_interpolation_amd as fi
    sizes = [side, side, side]
    nvox = side ** 3
    print("volume %d^3 (%d voxels), images %d x %d, %d images a launch" % (side, nvox, WIDTH, HEIGHT, fi._capi.FI_DEPTH_CAMERAS))
    src = torch.rand(2 * nvox, device="cuda")
    dst = torch.empty_like(src)
    timed("device copy of %.0f MB to another buffer (the bytes of one pass)" % (8 * nvox / 1e6), lambda: dst.copy_(src))
    for name, fov in (("wide", math.radians(50.0)), ("narrow", math.radians(12.0))):
        cams, depths = views(fi, side, fov)
        dev = [torch.from_numpy(d).cuda() for d in depths]
        incs = [fi.depth_to_points(c, d, positions=False, normals=False, valid=False)[0] for c, d in zip(cams, dev)]
        flat, flat_inc = torch.cat([d.reshape(-1) for d in dev]), torch.cat(incs)
        npix = WIDTH * HEIGHT
        vol = fi.DepthVolume(sizes, 4.0)
        for cull in (True, False):
            if cull:
                os.environ.pop("FI_NO_DEPTH_CULL", None)
            else:
                os.environ["FI_NO_DEPTH_CULL"] = "1"
            for m in (1, 4, 16):
                timed("%s views, %s, m = %2d, per image" % (name, "cull" if cull else "no cull", m),
                      lambda: vol.integrate(cams[:m], flat[:m * npix], flat_inc[:m * npix]), per=m)
            timed("%s views, %s, m = 16 without incidences, per image" % (name, "cull" if cull else "no cull"),
                  lambda: vol.integrate(cams, flat), per=16)
        os.environ.pop("FI_NO_DEPTH_CULL", None)
        for c in (1, 2, 4, 8):
            def chunks():
                for s in range(0, 16, c):
                    vol.integrate(cams[s:s + c], flat[s * npix:(s + c) * npix], flat_inc[s * npix:(s + c) * npix])
            timed("%s views, cull, 16 images handed over %d at a call, per image" % (name, c), chunks, per=16)
        seen = int((vol.weight(device=True) > 0).sum())
        print("%-74s %d of %d voxels seen" % ("", seen, nvox))
        if name == "wide":
            timed("depth_to_points of one image, every output", lambda: fi.depth_to_points(cams[0], dev[0], 2.0))
            out = timed("constraints(), device arrays", lambda: vol.constraints(device=True))
            print("%-74s %d band voxels" % ("", len(out[0])))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 256)
