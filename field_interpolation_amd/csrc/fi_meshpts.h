// fi_meshpts.h -- points spread over a device mesh by area and the deviation of a mesh from a surface (fi_meshpts.hip).  The
// contract is include/fi_hip.h (fi_mesh_sample, fi_mesh_deviation), DESIGN.md 4.17.
#pragma once

#include "fi_iso.h"
#include "fi_surface.h"

namespace fi {

void mesh_sample(const fi_mesh* m, long n, unsigned long long seed, int normals_mode, float* positions, float* normals,
                 long long* primitives, int memory);
void mesh_deviation(const fi_mesh* a, fi_surface* b, long samples, unsigned long long seed, float max_distance, fi_deviation* of_samples,
                    fi_deviation* of_vertices, float* vertex_distances, int memory);

}  // namespace fi
