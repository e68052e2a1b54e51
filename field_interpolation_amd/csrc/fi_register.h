// fi_register.h -- rigid registration of a point cloud to a mesh or to a point set on the device (fi_register.hip).  The
// contract is include/fi_hip.h (fi_mesh_register, fi_points_register), DESIGN.md 4.18.
#pragma once

#include "fi_iso.h"
#include "fi_nearest.h"
#include "fi_surface.h"

namespace fi {

// target may be null with an index and FI_REGISTER_POINT (a surface alone holds no vertices to take normals from); index null:
// built from target for the length of the call
void mesh_register(const fi_mesh* target, fi_surface* index, long n, const float* source, const fi_register_options* opt,
                   const double* initial, fi_registration* out, float* transformed, float* distances, int memory);
void points_register(const fi_points* target, const float* target_normals, long n, const float* source, const fi_register_options* opt,
                     const double* initial, fi_registration* out, float* transformed, float* distances, int memory);

}  // namespace fi
