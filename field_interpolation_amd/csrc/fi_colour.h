// fi_colour.h -- colour in a depth volume (fi_colour.hip): up to four planar fp32 channels and one colour weight per voxel,
// fused from colour images beside the depth images, sampled at points, rendered beside the depth image and handed out as data
// points per channel.  The contract is include/fi_hip.h (fi_volume_integrate_colour, fi_volume_colour_sample), DESIGN.md 4.29.
#pragma once

#include "fi_depth.h"

namespace fi {

constexpr int kMaxChannels = 4;

void volume_set_channels(fi_volume* v, int channels, hipStream_t st);  // allocates, colours = 0, colour weight = 0

// fi_volume_integrate's update of tsdf and weight, and the colours of the same images into the channels; every image buffer
// lives in `memory`, the cameras on the host
void volume_integrate_colour(fi_volume* v, long m, const fi_camera* cameras, const float* depths, const float* incidences,
                             const float* image_weights, float min_incidence, const float* colours, float band, int memory,
                             hipStream_t st);

// the colour at n points (3 floats each): colours float[n channels], valid (or null) unsigned char[n], in `memory`
void volume_colour_sample(const fi_volume* v, float min_weight, int64_t n, const float* positions, float* colours, unsigned char* valid,
                          int memory, hipStream_t st);

// march_image over the volume's tsdf and weight, then the colour at every hit position
void volume_render_colour(const fi_volume* v, const fi_march_options& o, const fi_camera& cam, float colour_min_weight, float* depth,
                          float* positions, float* normals, float* incidence, float* colours, int memory, hipStream_t st);

// the coloured voxels as data points: their count; with any of the outputs (of `capacity` points each, in `memory`) the arrays
int64_t volume_colour_constraints(const fi_volume* v, float min_weight, int64_t capacity, float* positions, float* colours, float* weights,
                                  int memory, hipStream_t st);

}  // namespace fi
