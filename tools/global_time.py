"""Times the coarse alignment (fi_feature.hip, fi_align.hip) on the device next to its yardsticks (profiles/global.md holds the
numbers).

    python tools/global_time.py config4 [side]   config 4's 1 M points uniformly random in its 256^3 lattice
    python tools/global_time.py config5 [side]   config 5's 5 M points on a sphere in its 512^3 lattice

The cloud is thinned on a grid (thin_points, the cell found by bisection) to about 100 000 points, its normals estimated at
k = 16; the second cloud is the first turned 97 degrees about (1, 2, 3) and shifted.  describe at k = 32 stands beside
neighbour_distances at k = 32: the same walk.  match_features is n x n pair evaluations of 33 columns.  The score is taken as
a difference: with the edge test off every hypothesis is scored, so (the call at 32768 trials - the call at 16384) is one
further batch of 16384 hypotheses over all pairs, the list of live pairs and the result's passes cancelled.  Inputs and outputs
are device tensors.  Every call is made once as a warm-up and REPS times between two HIP events; the figure is the median.
Nothing outside the tree is read."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cloud_time import points, timed  # noqa: E402

TARGET = 100_000


def thinned(fi, pd):
    lo, hi = 0.25, 64.0
    for _ in range(12):
        cell = (lo * hi) ** 0.5
        out = fi.thin_points(pd, cell)
        if len(out) > 1.05 * TARGET:
            lo = cell
        elif len(out) < 0.95 * TARGET:
            hi = cell
        else:
            break
    print("thinned at cell %.3f to %d points" % (cell, len(out)))
    return out


def cloud(kind, side):
    import torch

    import field_interpolation_amd as fi
    sizes, pos = points(kind, side)
    print("%s: %d points, lattice %s" % (kind, len(pos), "x".join(map(str, sizes))))
    tp = thinned(fi, torch.from_numpy(pos).cuda()).contiguous()
    n = len(tp)
    index = fi.PointIndex(tp)
    tn = index.estimate_normals(k=16, device=True)
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(97.0)
    R = torch.from_numpy((np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)).astype(np.float32)).cuda()
    sp = ((tp - torch.tensor([5.0, -3.0, 4.0], device=tp.device)) @ R).contiguous()
    sn = (tn @ R).contiguous()

    timed("neighbour_distances k = 32", lambda: index.neighbour_distances(32, device=True))
    ft, vt = timed("describe k = 32", lambda: index.describe(tn, 32))
    fs, vs = fi.PointIndex(sp).describe(sn, 32)
    print("%-58s %d of %d described" % ("", int(vt.sum()), n))
    matches = timed("match_features, %d x %d rows of 33" % (n, n), lambda: fi.match_features(fs, ft, vs, vt))
    right = int((matches == torch.arange(n, device=matches.device)).sum())
    print("%-58s %.3e pair evaluations; %d of %d matches are the point itself" % ("", float(n) * n, right, n))
    here = torch.arange(n, device=tp.device)
    one = timed("align_correspondences, 16384 trials, no edge test, no stop",
                lambda: fi.align_correspondences(sp, tp, here, matches, 1.0, 0.0, 16384, 0.0))
    two = timed("align_correspondences, 32768 trials, no edge test, no stop",
                lambda: fi.align_correspondences(sp, tp, here, matches, 1.0, 0.0, 32768, 0.0))
    assert one[0]["trials"] == 16384 and two[0]["trials"] == 32768
    print("%-58s %d and %d valid hypotheses x %d live pairs; best %d inliers" % ("", one[0]["valid"], two[0]["valid"], two[0]["live"],
                                                                                  two[0]["inliers"]))
    # pairs at random: the edge test at 0.9 refuses nearly every hypothesis, so a further batch is the models, the list of the
    # valid ones, a score grid whose groups leave at once, the keys and the read-back
    wrong = matches[torch.randperm(n, device=matches.device)]
    few = timed("random pairs, similarity 0.9, 16384 trials, no stop", lambda: fi.align_correspondences(sp, tp, here, wrong, 1.0, 0.9, 16384, 0.0))
    more = timed("random pairs, similarity 0.9, 65536 trials, no stop", lambda: fi.align_correspondences(sp, tp, here, wrong, 1.0, 0.9, 65536, 0.0))
    print("%-58s %d and %d valid hypotheses" % ("", few[0]["valid"], more[0]["valid"]))
    got = timed("align_correspondences, the default options", lambda: fi.align_correspondences(sp, tp, here, matches, 1.0))
    print("%-58s found %s, %d inliers, %d trials, %d valid" % ("", got[0]["found"], got[0]["inliers"], got[0]["trials"], got[0]["valid"]))
    both = timed("register_global, the default options", lambda: fi.register_global(sp, sn, tp, tn, 1.0))
    print("%-58s %d inliers, then %d steps to rms %.5f" % ("", both[0]["inliers"], both[1]["iterations"], both[1]["rms"]))


if __name__ == "__main__":
    cloud(sys.argv[1] if len(sys.argv) > 1 else "config4", int(sys.argv[2]) if len(sys.argv) > 2 else 0)
