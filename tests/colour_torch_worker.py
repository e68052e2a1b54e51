"""Worker of tests/test_gpu_colour.py::test_device_tensors, started as a fresh process: torch brings its own HIP runtime and
must stay out of the pytest process.  The depth, incidence and colour images, the image weights and the query points of
<in.npz> go to the device as torch tensors, through DepthVolume (integrate with colours, colours, colour_weight, load_colours,
sample_colours, colour_constraints, render with colours); the answers come back to <out.npz>.  The last camera of <in.npz> is
the one that renders."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
a = np.load(src)
cams = [fi.Camera(p, *k, int(s[0]), int(s[1]), "z" if s[2] == 0 else "range") for p, k, s in zip(a["pose"], a["intr"], a["shape"])]
cams, view = cams[:-1], cams[-1]
depths, incs, weights, colours, points = (torch.from_numpy(a[k]).cuda() for k in ("depths", "incs", "weights", "colours", "points"))
host = lambda x: x.cpu().numpy()  # noqa: E731
out, on_device = {}, []

sizes, channels = [20, 18, 16], 4
names = ("tsdf", "weight", "colours", "colour_weight")


def state(v):
    return v.tsdf(device=True), v.weight(device=True), v.colours(device=True), v.colour_weight(device=True)


vol = fi.DepthVolume(sizes, 2.5, 4.0, channels=channels)
vol.integrate(cams, depths, incs, weights, min_incidence=0.3, colours=colours)
got = state(vol)
on_device += [x.is_cuda for x in got]
for name, x in zip(names, got):
    out[name] = host(x)
# the colours again from an address one float past a 16-byte boundary: the kernel reads a pixel's channels one by one
room = torch.empty(colours.numel() + 4, dtype=torch.float32, device="cuda")
base = (-(room.data_ptr() // 4) % 4 + 1) % 4                     # element offset with (address / 4) % 4 == 1
shifted = room[base:base + colours.numel()]
assert shifted.data_ptr() % 16 == 4
shifted.copy_(colours)
other = fi.DepthVolume(sizes, 2.5, 4.0, channels=channels)
other.integrate(cams, depths, incs, weights, min_incidence=0.3, colours=shifted)
for name, x in zip(names, state(other)):
    out["shifted_" + name] = host(x)

# the state through load and load_colours, from device tensors, into a third volume: the queries go to that one
again = fi.DepthVolume(sizes, 2.5, 4.0, channels=channels).load(got[0], got[1]).load_colours(got[2], got[3])
col, valid = again.sample_colours(points, 0.5, valid=True)
on_device += [col.is_cuda, valid.is_cuda]
out["sample"], out["valid"] = host(col), host(valid)
con = again.colour_constraints(1.0, device=True)
on_device += [c.is_cuda for c in con]
for i, c in enumerate(con):
    out["con_%d" % i] = host(c)
img = again.render(view, positions=True, colours=True, device=True)
on_device += [x.is_cuda for x in img]
out["img_depth"], out["img_positions"], out["img_colours"] = (host(x) for x in img)
out["on_device"] = np.array(on_device)
np.savez(dst, **out)
print("colour torch worker done")
