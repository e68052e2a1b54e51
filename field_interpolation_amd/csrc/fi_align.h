// fi_align.h -- the rigid motion that most matched pairs of two point clouds agree on (fi_align.hip): RANSAC over
// correspondences with an exact inlier count, the coarse alignment in front of fi_register.hip's ICP.  No tree and no build:
// points and indices in `memory`, on the current device.  The contract is include/fi_hip.h (fi_align_correspondences),
// DESIGN.md 4.22.
#pragma once

#include <cstdint>

#include "fi_internal.h"

namespace fi {

// out (host) and inliers (m bytes in `memory`, or null) of the best rotation and shift over the m pairs
// (source[src_index[c]], target[tgt_index[c]]); source and target hold n_s and n_t points of 3 floats
void align_correspondences(int64_t n_s, const float* source, int64_t n_t, const float* target, int64_t m, const long long* src_index,
                           const long long* tgt_index, const fi_align_options& opt, fi_alignment* out, unsigned char* inliers, int memory);

}  // namespace fi
