// The dc:: drop-in (include/field_interpolation/dual_contouring_2d.hpp) over fi_dual_contour_field.
#include "field_interpolation/dual_contouring_2d.hpp"

#include <cstdio>

#include <fi_hip.h>

namespace dc {

void dual_contouring_2d(std::vector<Vec2>* out_vertices, std::vector<unsigned>* out_line_segments, size_t width, size_t height,
                        const float* distances, const Vec2* gradients)
{
	if (width < 2 || height < 2) { return; }
	const int sizes[2] = {static_cast<int>(width), static_cast<int>(height)};
	fi_mesh* m = nullptr;
	long nv = 0, np = 0;
	int vpp = 0;
	bool ok = fi_dual_contour_field(distances, reinterpret_cast<const float*>(gradients), 2, sizes, 0.0f, FI_HOST, &m) == FI_OK &&
	          fi_mesh_info(m, &nv, &np, &vpp) == FI_OK;
	std::vector<Vec2> v(static_cast<size_t>(nv));
	std::vector<int>  idx(2 * static_cast<size_t>(np));
	ok = ok && fi_mesh_copy(m, reinterpret_cast<float*>(v.data()), nullptr, idx.data(), nullptr, FI_HOST) == FI_OK;
	fi_mesh_destroy(m);
	if (!ok) {
		std::fprintf(stderr, "dc::dual_contouring_2d: %s\n", fi_last_error());
		return;
	}
	const unsigned first = static_cast<unsigned>(out_vertices->size());
	out_vertices->insert(out_vertices->end(), v.begin(), v.end());
	out_line_segments->reserve(out_line_segments->size() + idx.size());
	for (int i : idx) { out_line_segments->push_back(first + static_cast<unsigned>(i)); }
}

void calculate_gradients(Vec2* out_gradients, size_t width, size_t height, const float* distances)
{
	const auto at = [=](size_t x, size_t y) { return distances[y * width + x]; };
	for (size_t y = 0; y < height; ++y) {
		for (size_t x = 0; x < width; ++x) {
			Vec2& g = out_gradients[y * width + x];
			if (width < 2) {
				g.x = 0.0f;
			} else if (x == 0) {
				g.x = at(x + 1, y) - at(x, y);
			} else if (x == width - 1) {
				g.x = at(x, y) - at(x - 1, y);
			} else {
				g.x = (at(x + 1, y) - at(x - 1, y)) / 2;
			}
			if (height < 2) {
				g.y = 0.0f;
			} else if (y == 0) {
				g.y = at(x, y + 1) - at(x, y);
			} else if (y == height - 1) {
				g.y = at(x, y) - at(x, y - 1);
			} else {
				g.y = (at(x, y + 1) - at(x, y - 1)) / 2;
			}
		}
	}
}

}  // namespace dc
