// fi_depth.h -- depth images on the device (fi_depth.hip): a depth image unprojected into oriented points, and a truncated
// signed distance volume over a 3-D lattice that fuses depth images and hands its band to the solve as data points.  The
// contract is include/fi_hip.h (fi_depth_unproject, fi_volume_integrate), DESIGN.md 4.27.
#pragma once

#include "fi_internal.h"

struct fi_volume {
	int        device = 0;
	int        n[3]   = {0, 0, 0};
	int64_t    nvox   = 0;
	float      truncation = 0, max_weight = 0;
	fi::DevBuf tsdf, weight;  // float[nvox], x fastest
	// the optional colour state (fi_colour.hip; fi_volume_set_channels): nothing in fi_depth.hip or fi_march.hip touches it
	int        channels = 0;          // 0: none yet, else 1 .. 4
	fi::DevBuf colour, colour_weight;  // float[channels nvox], planar (channel k of voxel i at k nvox + i), and float[nvox]
};

namespace fi {

// the cameras of a call are host structures; every other buffer lives in `memory`
void check_camera(const fi_camera& cam);
int64_t camera_pixels(const fi_camera& cam);

void depth_unproject(const fi_camera& cam, const float* depth, float max_jump, float* positions, float* normals, float* incidence,
                     unsigned char* valid, int memory, hipStream_t st);

void volume_reset(fi_volume* v, hipStream_t st);  // tsdf = 1, weight = 0
void volume_integrate(fi_volume* v, long m, const fi_camera* cameras, const float* depths, const float* incidences,
                      const float* image_weights, float min_incidence, int memory, hipStream_t st);

// the band's voxels as data points: their count; with any of the outputs (of `capacity` points each, in `memory`) the arrays
int64_t volume_constraints(const fi_volume* v, float min_weight, int64_t capacity, float* positions, float* values, float* weights,
                           int memory, hipStream_t st);
// the same arrays in device buffers of the caller's (sized by this call); returns the count
int64_t volume_constraints_device(const fi_volume* v, float min_weight, DevBuf& positions, DevBuf& values, DevBuf& weights,
                                  hipStream_t st);

}  // namespace fi
