"""Times the plane segmentation (fi_plane.hip) on the device next to its yardstick, fi_cluster_measure of the same points
(profiles/plane.md holds the numbers).

    python tools/plane_time.py config4 [side]   config 4's 1 M points uniformly random in its 256^3 lattice
    python tools/plane_time.py config5 [side]   config 5's 5 M points on a sphere in its 512^3 lattice
    python tools/plane_time.py split [side]     config 4, a default call and a four-batch call once each after a warm-up and
                                                nothing else: the run to put under `rocprofv3 --kernel-trace --stats` for
                                                the kernels' shares

Neither cloud holds a plane, so no call stops early: a call at max_trials = T scores T hypotheses.  One batch's score is taken
as a difference: (the call at 4096 trials - the call at 1024 trials) / 3 is one further batch -- 1024 models, the score, the key
and the batch's read-back -- with the candidate list, the flags and the result's passes cancelled.  The threshold is half a
lattice unit.  Inputs and outputs are device tensors.  Every call is made once as a warm-up and REPS times between two HIP
events on the stream the library works on; the figure is the median of the REPS event times, with the fastest and the slowest
beside it.  Nothing outside the tree is read."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cloud_time import points, timed  # noqa: E402

THRESHOLD = 0.5


def cloud(kind, side, split=False):
    import torch

    import field_interpolation_amd as fi
    sizes, pos = points(kind, side)
    n = len(pos)
    print("%s: %d points, lattice %s" % (kind, n, "x".join(map(str, sizes))))
    pd = torch.from_numpy(pos).cuda()
    if split:
        run = lambda label, fn: fn()  # noqa: E731
        fi.segment_plane(pd, THRESHOLD)                       # warm-up: the allocations
        torch.cuda.synchronize()
    else:
        run = timed
    model, inliers = run("segment_plane, the default options (1024 trials, 2 refits)", lambda: fi.segment_plane(pd, THRESHOLD))
    print("%-58s %d inliers of %d, %d trials, %d refits, rms %.4f" % ("", model["inliers"], n, model["trials"], model["refits"], model["rms"]))
    one = run("segment_plane, 1024 trials, no refit, no stop", lambda: fi.segment_plane(pd, THRESHOLD, 1024, 0.0, 0))
    four = run("segment_plane, 4096 trials, no refit, no stop", lambda: fi.segment_plane(pd, THRESHOLD, 4096, 0.0, 0))
    assert one[0]["trials"] == 1024 and four[0]["trials"] == 4096 and four[0]["inliers"] >= one[0]["inliers"]
    if split:
        return
    labels, models = run("segment_planes, 2 planes, the default options", lambda: fi.segment_planes(pd, THRESHOLD, 2))
    print("%-58s %s inliers" % ("", [m["inliers"] for m in models]))
    every = torch.zeros(n, dtype=torch.int32, device=pd.device)
    rows = run("cluster_measure of the same points as one cluster", lambda: fi.cluster_measure(pd, every, num_clusters=1))
    assert rows[0]["count"] == n


if __name__ == "__main__":
    kind = sys.argv[1] if len(sys.argv) > 1 else "config4"
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    cloud("config4" if kind == "split" else kind, side, split=kind == "split")
