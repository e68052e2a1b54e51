// dual_contouring_2d.hpp -- drop-in for src/dual_contouring_2d.hpp of emilk/field_interpolation.
//
// Same namespace, names and signatures as the reference header, written for this project: dual_contouring_2d runs on the
// GPU through libfi_hip (include/fi_hip.h fi_dual_contour_field, whose contract restates the reference's arithmetic so that
// the output is the reference's, bit for bit, wherever its fit ends finite within 32 solves).  Differences:
//   - calculate_gradients takes the y border at height - 1 (the reference tests width - 1 and reads out of bounds on
//     non-square lattices);
//   - a non-finite distance, or a failure of the library, leaves the outputs as they were and prints the library's message.
#pragma once

#include <cstddef>
#include <vector>

namespace dc {

using Index = unsigned;

struct Vec2 { float x, y; };
static_assert(sizeof(Vec2) == sizeof(float) * 2, "Pack");

// Line segments where `distances` (width * height, x fastest; <= 0 inside) crosses zero: one vertex per crossed cell, appended
// to *out_vertices; index pairs (into *out_vertices, after what it held before) appended to *out_line_segments, with the
// inside on their left.  gradients: width * height local gradients of the distances (e.g. from calculate_gradients).
void dual_contouring_2d(std::vector<Vec2>* out_vertices, std::vector<unsigned>* out_line_segments, size_t width, size_t height,
                        const float* distances, const Vec2* gradients);

// Central differences (d[+1] - d[-1]) / 2 per axis, one-sided at that axis's border.  Computed on the host.
void calculate_gradients(Vec2* out_gradients, size_t width, size_t height, const float* distances);

}  // namespace dc
