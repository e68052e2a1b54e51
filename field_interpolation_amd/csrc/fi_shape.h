// fi_shape.h -- the spheres (circles in 2-D) and cylinders of a point cloud on the device (fi_shape.hip): RANSAC with an exact
// inlier count and algebraic least-squares refits, one shape or several peeled off in turn.  No tree and no build: positions
// and normals in `memory`, on the current device.  The contract is include/fi_hip.h (fi_shape_fit and what follows it),
// DESIGN.md 4.26.
#pragma once

#include <cstdint>

#include "fi_internal.h"

namespace fi {

// model (host) and inliers (n bytes in `memory`, or null) of the best shape of opt.kind through the candidates among n
// positions of ndim (2 or 3) floats; normals (as the positions) and mask (n bytes) in `memory`, or null
void shape_fit(int ndim, int64_t n, const float* positions, const float* normals, const unsigned char* mask, const fi_shape_options& opt,
               fi_shape_model* model, unsigned char* inliers, int memory);

// labels (n ints in `memory`), rows (host, max_shapes) and *num_shapes: shape p is shape_fit with seed + p over the
// candidates no earlier shape took, until max_shapes, no shape, or a shape of fewer than min_inliers points
void shapes_segment(int ndim, int64_t n, const float* positions, const float* normals, const unsigned char* mask, const fi_shape_options& opt,
                    int max_shapes, int64_t min_inliers, int* labels, fi_shape_model* rows, int* num_shapes, int memory);

}  // namespace fi
