// fi_plane.h -- the dominant hyperplanes of a point cloud on the device (fi_plane.hip): RANSAC with an exact inlier count
// and least-squares refits, one plane or several peeled off in turn.  No tree and no build: positions in `memory`, on the
// current device.  The contract is include/fi_hip.h (fi_plane_fit and what follows it), DESIGN.md 4.21.
#pragma once

#include <cstdint>

#include "fi_internal.h"

namespace fi {

// model (host) and inliers (n bytes in `memory`, or null) of the best hyperplane through the candidates among n positions of
// ndim (2 or 3) floats; mask (n bytes in `memory`) or null
void plane_fit(int ndim, int64_t n, const float* positions, const unsigned char* mask, const fi_plane_options& opt, fi_plane_model* model,
               unsigned char* inliers, int memory);

// labels (n ints in `memory`), rows (host, max_planes) and *num_planes: plane p is plane_fit with seed + p over the
// candidates no earlier plane took, until max_planes, no plane, or a plane of fewer than min_inliers points
void planes_segment(int ndim, int64_t n, const float* positions, const unsigned char* mask, const fi_plane_options& opt, int max_planes,
                    int64_t min_inliers, int* labels, fi_plane_model* rows, int* num_planes, int memory);

}  // namespace fi
