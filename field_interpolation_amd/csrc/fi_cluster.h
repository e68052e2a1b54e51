// fi_cluster.h -- the clusters of a point cloud on the device (fi_cluster.hip): Euclidean clusters and DBSCAN labels over
// fi_nearest.h's tree (no tree and no build of their own), and a table per cluster that needs no tree.  The contract is
// include/fi_hip.h (fi_cluster and what follows it), DESIGN.md 4.20.
#pragma once

#include "fi_nearest.h"

namespace fi {

// labels (t.n ints in `memory`, or null), core (t.n bytes in `memory`, or null) and stats (host, or null) of the set's own
// points: core points by min_points within eps, clusters of core points numbered by their lowest core point, border points
// by their nearest core point, -1 for the rest
void cluster_labels(const NearestIndex& t, float eps, int min_points, int* labels, unsigned char* core, fi_cluster_stats* stats,
                    int memory, hipStream_t st);

// rows (host, num_clusters) of the clusters that `labels` (n ints) names among n positions of ndim floats; core (n bytes) or
// null; positions, labels and core in `memory`; on the current device
void cluster_measure(int ndim, int64_t n, const float* positions, const int* labels, const unsigned char* core, int64_t num_clusters,
                     fi_cluster_row* rows, int memory);

}  // namespace fi
