"""Times the colour unit (fi_colour.hip) on the device next to its yardsticks (profiles/colour.md is where the numbers go):
DepthVolume.integrate of m = 1, 4, 16 range images of 640 x 480 into a side^3 volume (default 256) with colours at C = 3 and
C = 4 channels, and without colours on the same images beside them; a plain device copy of the bytes one pass over the volume
moves (tsdf, W, Wc and C channels read and written: 2 (3 + C) 4 B a voxel, against 16 B without colours); sample_colours of
1 M points; and render with and without colours at 1024 x 1024.

    python tools/colour_time.py [side]

Inputs are device tensors.  Every call is made once as a warm-up; a window is INNER calls back to back between two HIP events
on the stream the library works on, and the figure is the median over REPS windows of the time per call, with the fastest and
the slowest window beside it.  A call includes what the library does on the host: staging the camera table and the stream
synchronise every entry point ends with.  Nothing outside the tree is read."""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 9
INNER = 20
WIDTH, HEIGHT = 640, 480


def timed(label, fn, per=1, inner=INNER):
    import torch
    fn()  # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / (per * inner))
    print("%-78s median of %d x %d: %8.3f ms (min %.3f, max %.3f)" % (label, REPS, inner, statistics.median(ms), min(ms), max(ms)))
    return out


def views(fi, side, count=16):
    """count cameras (fov 50 degrees) around a sphere of radius 0.3 side in the middle of the lattice: its range images and
    colour images (4 channels, a smooth function of the surface point; the first 3 serve C = 3)"""
    import numpy as np
    centre = np.full(3, 0.5 * (side - 1))
    rng = np.random.default_rng(2)
    cams, depths, colours = [], [], []
    for _ in range(count):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        eye = centre + 1.3 * side * d
        cam = fi.camera_look_at(eye, centre, np.cross(d, rng.normal(size=3)), math.radians(50.0), WIDTH, HEIGHT)
        R, t = cam.pose[:, :3].astype(np.float64), cam.pose[:, 3].astype(np.float64)
        rows, cols = np.meshgrid(np.arange(HEIGHT), np.arange(WIDTH), indexing="ij")
        ray = np.stack([(cols + 0.5 - cam.cx) / cam.fx, (rows + 0.5 - cam.cy) / cam.fy, np.ones(rows.shape)], axis=-1)
        ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
        ray = ray @ R
        oc = -R.T @ t - centre
        b = ray @ oc
        disc = b * b - (oc @ oc - (0.3 * side) ** 2)
        hit = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), np.inf)
        u = (oc + np.where(np.isfinite(hit), hit, 0.0)[..., None] * ray) / (0.3 * side)
        colour = np.stack([0.5 + 0.4 * u[..., 0], 0.5 + 0.3 * u[..., 1], 0.5 + 0.4 * u[..., 2], 0.5 + 0.5 * u[..., 0] * u[..., 1]], axis=-1)
        cams.append(cam)
        depths.append(hit.astype(np.float32))
        colours.append(np.where(np.isfinite(hit)[..., None], colour, np.nan).astype(np.float32))
    return cams, depths, colours


def main(side):
    import numpy as np
    import torch

    import field_interpolation_amd as fi
    sizes = [side, side, side]
    nvox = side ** 3
    npix = WIDTH * HEIGHT
    print("volume %d^3 (%d voxels), images %d x %d, %d images a launch" % (side, nvox, WIDTH, HEIGHT, fi._capi.FI_DEPTH_CAMERAS))
    cams, depths, colours = views(fi, side)
    dev = [torch.from_numpy(d).cuda() for d in depths]
    incs = [fi.depth_to_points(c, d, positions=False, normals=False, valid=False)[0] for c, d in zip(cams, dev)]
    flat, flat_inc = torch.cat([d.reshape(-1) for d in dev]), torch.cat(incs)
    for floats in (4, 6, 7):                                            # tsdf + W, and + Wc + C channels
        src = torch.rand(floats * nvox, device="cuda")
        dst = torch.empty_like(src)
        timed("device copy of %.0f MB to another buffer (one pass: %d B a voxel read and written)" % (4 * floats * nvox / 1e6, 8 * floats),
              lambda: dst.copy_(src))
        del src, dst
    plain = fi.DepthVolume(sizes, 4.0)
    for m in (1, 4, 16):
        timed("integrate without colours, m = %2d, per image" % m, lambda: plain.integrate(cams[:m], flat[:m * npix], flat_inc[:m * npix]), per=m)
    del plain
    vol = None
    for channels in (3, 4):
        col = torch.cat([torch.from_numpy(np.ascontiguousarray(c[..., :channels])).cuda().reshape(-1) for c in colours])
        vol = fi.DepthVolume(sizes, 4.0, channels=channels)
        for m in (1, 4, 16):
            timed("integrate with colours, C = %d, m = %2d, per image" % (channels, m),
                  lambda: vol.integrate(cams[:m], flat[:m * npix], flat_inc[:m * npix], colours=col[:m * npix * channels]), per=m)
        print("%-78s %d of %d voxels coloured" % ("", int((vol.colour_weight(device=True) > 0).sum()), nvox))
        del col
    # (vol: the C = 4 volume after 16 wide views)
    centre = 0.5 * (side - 1)
    u = torch.randn(1_000_000, 3, device="cuda")
    pts = (centre + 0.3 * side * u / u.norm(dim=1, keepdim=True)).float().contiguous()
    out = timed("sample_colours of 1 M points of the sphere, C = 4", lambda: vol.sample_colours(pts, valid=True))
    print("%-78s %d of %d samples valid" % ("", int(out[1].sum()), len(pts)))
    cam = fi.camera_look_at([centre + 1.3 * side, centre + 0.2 * side, centre + 0.3 * side], [centre] * 3, (0.0, 0.0, 1.0), math.radians(50.0),
                            1024, 1024)
    timed("render 1024 x 1024, depth and positions", lambda: vol.render(cam, positions=True, device=True), inner=5)
    out = timed("render 1024 x 1024, depth, positions and colours, C = 4", lambda: vol.render(cam, positions=True, colours=True, device=True),
                inner=5)
    print("%-78s %d of %d pixels hit, %d coloured" % ("", int(torch.isfinite(out[0]).sum()), 1024 * 1024, int(torch.isfinite(out[2][:, 0]).sum())))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 256)
