// fi_smooth.h -- Taubin fairing of a device mesh and normals recomputed from its primitives (fi_smooth.hip).  The contract is
// include/fi_hip.h (fi_mesh_smooth, fi_mesh_normals), DESIGN.md 4.16.
#pragma once

#include "fi_iso.h"

namespace fi {

void mesh_smooth(const fi_mesh* m, const fi_smooth_options* opt, fi_mesh** out);
void mesh_normals(const fi_mesh* m, fi_mesh** out);

}  // namespace fi
