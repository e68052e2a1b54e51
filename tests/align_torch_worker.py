"""Worker of tests/test_gpu_align.py::test_device_tensors and tests/test_gpu_feature.py::test_device_tensors, started as a
fresh process: torch brings its own HIP runtime and must stay out of the pytest process.  The two scans of <in.npz> go to the
device as torch tensors, through PointIndex.describe, match_features, align_correspondences and register_global; the
answers come back to <out.npz>."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import field_interpolation_amd as fi  # noqa: E402

src, dst = sys.argv[1], sys.argv[2]
data = np.load(src)
sp, sn, tp, tn = (torch.from_numpy(data[k]).cuda() for k in ("sp", "sn", "tp", "tn"))
host = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)  # noqa: E731

fs, vs = fi.PointIndex(sp).describe(sn, 32)
ft, vt = fi.PointIndex(tp).describe(tn, 32)
on_device = [fs.is_cuda, fs.dtype == torch.float32, vs.is_cuda, vs.dtype == torch.bool]
matches, distances = fi.match_features(fs, ft, vs, vt, distances=True)
mutual = fi.match_features(fs, ft, vs, vt, mutual=True)
on_device += [matches.is_cuda, matches.dtype == torch.int64, distances.is_cuda, mutual.is_cuda]
here = torch.arange(len(sp), device=sp.device)
result, mask = fi.align_correspondences(sp, tp, here, matches, 1.0, max_trials=16384, confidence=0.0)
on_device += [mask.is_cuda, mask.dtype == torch.bool]
alignment, registration = fi.register_global(sp, sn, tp, tn, 1.0, max_trials=16384, confidence=0.0)
on_device += [alignment["mask"].is_cuda, alignment["matches"].is_cuda, bool(torch.equal(alignment["matches"], matches)),
              bool(torch.equal(alignment["mask"], mask)), alignment["transform"].tobytes() == result["transform"].tobytes()]
np.savez(dst, features=host(fs), valid=host(vs), matches=host(matches), distances=host(distances), mutual=host(mutual), mask=host(mask),
         ints=np.array([int(result[k]) for k in ("found", "pairs", "live", "trials", "valid", "inliers")]),
         doubles=np.array(list(result["transform"].ravel()) + [result["rms"]]), refined=registration["transform"],
         on_device=np.array(on_device))
print("align torch worker done")
