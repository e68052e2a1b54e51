// fi_march.h -- rays and pinhole images of a lattice field or a depth volume (fi_march.hip): a ray is marched through the
// trilinear interpolant to the first crossing of an iso-level, with the unit gradient as the hit's normal.  The contract is
// include/fi_hip.h (fi_field_raycast, fi_field_render), DESIGN.md 4.28.
#pragma once

#include "fi_internal.h"

namespace fi {

// the field a call marches: device pointers, fp32, x fastest; w is null or the weight array of the same shape
struct MarchField {
	const float* f;
	const float* w;
	int          ndim;
	int          n[3];  // (1 beyond ndim)
};

// ndim 2 or 3, sizes >= 2, fewer than 2^31 lattice points; returns their number
int64_t check_march_field(int ndim, const int* sizes);
void    check_march_options(const fi_march_options* o);

// every ray buffer and output lives in `memory`; the field is on the device already
void march_rays(const MarchField& field, const fi_march_options& o, int64_t n, const float* origins, const float* directions,
                float t_min, float t_max, float* t, float* positions, float* normals, signed char* side, int memory, hipStream_t st);
void march_image(const MarchField& field, const fi_march_options& o, const fi_camera& cam, float* depth, float* positions,
                 float* normals, float* incidence, int memory, hipStream_t st);

}  // namespace fi
