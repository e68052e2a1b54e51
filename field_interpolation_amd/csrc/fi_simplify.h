// fi_simplify.h -- simplification of a device mesh by vertex clustering with quadric placement (fi_simplify.hip).  The
// contract is include/fi_hip.h (fi_mesh_simplify), DESIGN.md 4.15.
#pragma once

#include "fi_iso.h"

namespace fi {

// origin: ndim floats on the host, or null for 0; vertex_map: int32 per input vertex in `memory`, or null
void mesh_simplify(const fi_mesh* m, float cell, const float* origin, int placement, int* vertex_map, int memory, fi_mesh** out);

}  // namespace fi
