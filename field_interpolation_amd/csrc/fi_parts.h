// fi_parts.h -- the connected parts of a device mesh (fi_parts.hip): labels, per-part counts and measures, and the
// sub-mesh of chosen parts.  The contract is include/fi_hip.h (fi_mesh_create .. fi_mesh_select), DESIGN.md 4.13.
#pragma once

#include "fi_iso.h"

namespace fi {

// a caller's mesh (arrays in `memory`; normals / keys may be null)
void mesh_create(fi_mesh** out, int ndim, long num_vertices, const float* vertices, const float* normals, const long long* keys,
                 long num_primitives, const int* indices, int memory);
// labels into the caller's arrays in `memory` (either may be null)
void mesh_parts(const fi_mesh* m, long* num_parts, int* vertex_labels, int* primitive_labels, int memory);
// one row per part, on the host
void mesh_measure(const fi_mesh* m, long capacity, fi_mesh_part* parts, long* num_parts);
// the parts whose byte of keep (host) is set, as a new mesh
void mesh_select(const fi_mesh* m, long num_parts, const unsigned char* keep, fi_mesh** out);

}  // namespace fi
