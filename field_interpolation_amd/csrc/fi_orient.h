// fi_orient.h -- a consistent sign for point-cloud normals on the device (fi_orient.hip): the minimum spanning forest of the
// k-nearest-neighbour graph by Boruvka rounds, over the search structure of fi_nearest.h and the queries of fi_knn.h.
#pragma once

#include "fi_knn.h"

namespace fi {

// what a call did, for the profile notes (profiles/orient.md): with FI_ORIENT_STATS in the environment every call prints
// them on stderr (tools/orient_time.py); the events that time the parts are recorded only then
struct OrientStats {
	int    rounds           = 0;  // Boruvka rounds, the last one (which hooks nothing) included
	int    launches_a_round = 0;
	double table_ms         = 0;  // the neighbour table
	double propagate_ms     = 0;  // everything after it
};

// The normals of the set's own points (include/fi_hip.h fi_orient_normals): normals (t.n x D) read and written in place,
// components (t.n, or null), guides (num_guides x D) per `anchor`; every buffer in `memory`.
void orient_normals(const NearestIndex& t, int k, float max_distance, int anchor, const float* guides, int64_t num_guides,
                    float* normals, long long* components, int memory, hipStream_t st, OrientStats* stats = nullptr);

}  // namespace fi
