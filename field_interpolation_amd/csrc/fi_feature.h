// fi_feature.h -- descriptors of a point's neighbourhood that survive a rigid motion, and their matching (fi_feature.hip),
// over the search structure of fi_nearest.h: no tree and no build of its own.  The contract is include/fi_hip.h
// (fi_points_describe, fi_feature_match), DESIGN.md 4.22.
#pragma once

#include "fi_nearest.h"

namespace fi {

// features (t.n x 33) and valid (t.n bytes, or null) of the set's own points from their normals (t.n x 3), in point order;
// every buffer in `memory`.  3-D sets only.
void points_describe(const NearestIndex& t, const float* normals, int k, float max_distance, float* features, unsigned char* valid,
                     int memory, hipStream_t st);

// indices (n_a) and distances (n_a, or null): the nearest admissible row of b (n_b x dim) for every row of a (n_a x dim);
// valid_a / valid_b (one byte a row) or null; every buffer in `memory`, on the current device
void feature_match(int dim, int64_t n_a, const float* a, const unsigned char* valid_a, int64_t n_b, const float* b,
                   const unsigned char* valid_b, long long* indices, float* distances, int memory);

}  // namespace fi
