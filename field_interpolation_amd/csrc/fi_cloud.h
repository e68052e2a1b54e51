// fi_cloud.h -- a point cloud made clean on the device (fi_cloud.hip): how many points lie within a radius, how far a set's
// own points lie from their neighbours, the outlier masks built on the two, and thinning on a uniform grid.  The contract is
// include/fi_hip.h (fi_radius_count and what follows it), DESIGN.md 4.19.  The first four walk fi_nearest.h's tree: no tree
// and no build of their own.
#pragma once

#include "fi_nearest.h"

namespace fi {

// counts (n) of the points within `radius` of each of n queries, at most `limit`; queries and counts in `memory`
void cloud_radius_count(const NearestIndex& t, int64_t n, const float* queries, float radius, int limit, int* counts, int memory,
                        hipStream_t st);

// the set's own points, each over its k nearest other points within max_distance: mean, kth, counts (t.n each, any but not
// all of them null) in point order, in `memory`
void cloud_neighbour_distances(const NearestIndex& t, int k, float max_distance, float* mean, float* kth, int* counts, int memory,
                               hipStream_t st);

// keep (t.n bytes in `memory`, or null) and stats (host, or null) of the statistical rule over cloud_neighbour_distances' mean
void cloud_outliers_statistical(const NearestIndex& t, int k, float max_distance, float std_ratio, unsigned char* keep,
                                fi_outlier_stats* stats, int memory, hipStream_t st);

// keep (t.n bytes in `memory`, or null) and *num_kept (host, or null): the points with min_neighbours others within radius
void cloud_outliers_radius(const NearestIndex& t, float radius, int min_neighbours, unsigned char* keep, long* num_kept, int memory,
                           hipStream_t st);

// one output point per occupied cell of a uniform grid (include/fi_hip.h fi_cloud_thin); on the current device
void cloud_thin(int ndim, int64_t n, const float* positions, const float* normals, const float* values, float cell, const float* origin,
                int mode, float* out_positions, float* out_normals, float* out_values, int* out_counts, long long* out_indices,
                int* cell_map, long* num_out, int memory);

}  // namespace fi
