// fi_ray.h -- rays against a segment (2-D) or triangle (3-D) mesh on the device: closest hits, crossing counts, containment
// and the sign of the surface distances (fi_ray.hip), over the search structure fi_surface.hip builds; shared by the C ABI
// unit (fi_capi.hip).
#pragma once

#include "fi_surface.h"

namespace fi {

// The queries of the C ABI (include/fi_hip.h fi_surface_raycast): n rays (origins, directions: n x D floats) and the
// outputs in `memory`; primitives and bary (n x (D - 1) floats) may be null.
void ray_cast(const SurfaceIndex& t, int64_t n, const float* origins, const float* directions, float t_min, float t_max, float* hit_t,
              long long* primitives, float* bary, int memory, hipStream_t st);
// the hits of each ray in [t_min, t_max], saturated at limit >= 1
void ray_count(const SurfaceIndex& t, int64_t n, const float* origins, const float* directions, float t_min, float t_max, int limit,
               int* counts, int memory, hipStream_t st);
// inside[i] = the parity of the hits of the ray from points[i] along `direction` (D floats on the host; null: +x), t in [0, +inf)
void ray_contains(const SurfaceIndex& t, int64_t n, const float* points, const float* direction, unsigned char* inside, int memory,
                  hipStream_t st);
// surface_query / surface_lattice (fi_surface.hip, unchanged), their distances negated where the parity along +x is odd
void ray_signed_query(const SurfaceIndex& t, int64_t n, const float* queries, float max_distance, float* distances,
                      long long* primitives, float* closest, int memory, hipStream_t st);
void ray_signed_lattice(const SurfaceIndex& t, const int* sizes, float max_distance, float* out, long long* primitives, int memory,
                        hipStream_t st);

}  // namespace fi
