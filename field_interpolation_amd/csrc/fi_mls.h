// fi_mls.h -- a point cloud made smooth on the device (fi_mls.hip): every query projected onto the plane or quadric fitted to
// its weighted neighbours, with that surface's normal and curvature.  The contract is include/fi_hip.h (fi_mls_project),
// DESIGN.md 4.25.  It walks fi_nearest.h's tree: no tree and no build of its own.
#pragma once

#include "fi_nearest.h"

namespace fi {

// n queries (n x D), or with queries == nullptr the set's own t.n points; guide_normals (one per query, or null); positions,
// normals (n x D each), curvature (n), order (n bytes): any but not all of them null; every buffer in `memory`
void mls_project(const NearestIndex& t, int64_t n, const float* queries, int k, float radius, int degree, float max_move,
                 const float* guide_normals, float* positions, float* normals, float* curvature, unsigned char* order, int memory,
                 hipStream_t st);

}  // namespace fi
