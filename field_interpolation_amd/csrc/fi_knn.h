// fi_knn.h -- exact k nearest data points and point-cloud normals on the device (fi_knn.hip), over the search structure of
// fi_nearest.h: no tree and no build of its own.
#pragma once

#include "fi_nearest.h"

namespace fi {

constexpr int kMaxNeighbours = 32;

// The queries of the C ABI (include/fi_hip.h fi_knn): queries / distances (n x k) / indices (n x k, or null) in `memory`.
void knn_query(const NearestIndex& t, int64_t n, const float* queries, int k, float max_distance, float* distances, long long* indices,
               int memory, hipStream_t st);

// The normals of the set's own points (include/fi_hip.h fi_estimate_normals): normals (t.n x D) and variation (t.n, or null)
// in point order; guides (num_guides x D) per `orient`; every buffer in `memory`.
void estimate_normals(const NearestIndex& t, int k, float max_distance, int orient, const float* guides, int64_t num_guides,
                      float* normals, float* variation, int memory, hipStream_t st);

}  // namespace fi
