"""Times the sphere and cylinder segmentation (fi_shape.hip) on the device next to its yardstick, the plane segmentation of the
same points in the same run (profiles/shape.md holds the numbers).

    python tools/shape_time.py config4 [side]   config 4's 1 M points uniformly random in its 256^3 lattice
    python tools/shape_time.py config5 [side]   config 5's 5 M points on a sphere in its 512^3 lattice

Every point gets a random normal (a fixed seed), so no cloud holds a cylinder and config 4 holds no sphere either.  A call with
confidence = 0 never stops early: a call at max_trials = T scores T hypotheses, and one batch's cost is taken as a difference,
(the call at 4096 trials - the call at 1024 trials) / 3, as tools/plane_time.py does.  The threshold is half a lattice unit.
Inputs and outputs are device tensors.  Every call is made once as a warm-up and REPS times between two HIP events on the
stream the library works on; the figure is the median of the REPS event times, with the fastest and the slowest beside it.
Nothing outside the tree is read."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cloud_time import points, timed  # noqa: E402

THRESHOLD = 0.5


def cloud(kind, side):
    import numpy as np
    import torch

    import field_interpolation_amd as fi
    sizes, pos = points(kind, side)
    n = len(pos)
    print("%s: %d points, lattice %s" % (kind, n, "x".join(map(str, sizes))))
    pd = torch.from_numpy(pos).cuda()
    nd = torch.from_numpy(np.random.default_rng(9).normal(size=pos.shape).astype(np.float32)).cuda()

    def report(model):
        print("%-58s %d inliers of %d, %d trials, %d refits, radius %.3f, rms %.4f"
              % ("", model["inliers"], n, model["trials"], model["refits"], model["radius"], model["rms"]))

    calls = (("segment_sphere", lambda **kw: fi.segment_sphere(pd, THRESHOLD, **kw)),
             ("segment_sphere with normals, 20 degrees", lambda **kw: fi.segment_sphere(pd, THRESHOLD, normals=nd, max_angle=20.0, **kw)),
             ("segment_cylinder", lambda **kw: fi.segment_cylinder(pd, nd, THRESHOLD, **kw)),
             ("segment_cylinder, 20 degrees", lambda **kw: fi.segment_cylinder(pd, nd, THRESHOLD, max_angle=20.0, **kw)))
    for name, call in calls:
        model, _ = timed("%s, the default options" % name, call)
        report(model)
        one = timed("%s, 1024 trials, no refit, no stop" % name, lambda: call(max_trials=1024, confidence=0.0, refine=0))
        four = timed("%s, 4096 trials, no refit, no stop" % name, lambda: call(max_trials=4096, confidence=0.0, refine=0))
        assert one[0]["trials"] == 1024 and four[0]["trials"] == 4096 and four[0]["inliers"] >= one[0]["inliers"]
    model, _ = timed("segment_plane, the default options", lambda: fi.segment_plane(pd, THRESHOLD))
    print("%-58s %d inliers of %d, %d trials, %d refits" % ("", model["inliers"], n, model["trials"], model["refits"]))
    timed("segment_plane, 1024 trials, no refit, no stop", lambda: fi.segment_plane(pd, THRESHOLD, 1024, 0.0, 0))
    timed("segment_plane, 4096 trials, no refit, no stop", lambda: fi.segment_plane(pd, THRESHOLD, 4096, 0.0, 0))


if __name__ == "__main__":
    cloud(sys.argv[1] if len(sys.argv) > 1 else "config4", int(sys.argv[2]) if len(sys.argv) > 2 else 0)
