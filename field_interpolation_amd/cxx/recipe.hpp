// recipe.hpp (internal to libfield_interpolation) -- how a LinearEquation's rows were made, recorded beside the rows.
//
// The reference's application calls sdf_from_points(...) and then solve_tiled_with_guess(field.eq, ...) (src/sdf_field.cpp:251-304):
// only `eq` reaches the solver, a COO list of every model row of the lattice (config 3: 100 M triplets, 1.2 GB).  The row
// builders of this library (add_field_constraints, add_points) note WHAT they appended -- model weights, or copies of the
// point arrays -- and where (row / triplet ranges, a checksum of those triplets and right-hand sides); the solvers use the
// matrix-free lattice path (fi_set_model + fi_add_points, the stencil kernels) for the ranges that are still as recorded and
// upload only the rows nobody vouches for as triplets (fi_add_rows_coo).  A caller that edits the recorded rows in place fails
// the checksum and gets the generic path, as before: the checksum reads EVERY triplet and EVERY right-hand side of a noted
// range, when the range is noted and again at every solve (range_checksum below), so `eq` stays what the reference's
// callers take it for -- a public aggregate they may write into -- and nobody has to know about the note.  The header stays
// source-compatible: LinearEquation gains a trailing shared_ptr.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "field_interpolation/field_interpolation.hpp"

namespace field_interpolation {
namespace detail {

struct Segment {
	enum Kind { kModel, kPoints } kind = kModel;
	size_t row0 = 0, row1 = 0, trip0 = 0, trip1 = 0;  // the rows / triplets this call appended
	uint64_t checksum = 0;                            // range_checksum of the triplets [trip0, trip1) and the right-hand sides [row0, row1)
	Weights weights;                                  // kModel
	float value_weight = 0, gradient_weight = 0;      // kPoints
	ValueKernel value_kernel = ValueKernel::kLinearInterpolation;
	GradientKernel gradient_kernel = GradientKernel::kCellEdges;
	int num_points = 0;
	std::vector<float> positions, normals, point_weights;  // copies (normals / point_weights empty when null)
};

struct Recipe {
	std::vector<int>     sizes;
	std::vector<Segment> segments;
};

// All `bytes` bytes at p (a multiple of 4), in order, into h: four independent multiply-rotate lanes over 8-byte words, folded
// by mix_lanes.  Every step is a bijection of its lane for a fixed word and of the word for a fixed lane, so a change
// confined to one word always changes the result; anything else (a shifted tail after an insertion, two edits) goes
// unnoticed with a probability of about 2^-64.  Accidental edits are the threat, not adversaries.
inline void mix_bytes(uint64_t h[4], const unsigned char* p, size_t bytes)
{
	static const uint64_t K[4] = {0x9E3779B97F4A7C15ull, 0xC2B2AE3D27D4EB4Full, 0x165667B19E3779F9ull, 0xD6E8FEB86659FD93ull};
	auto step = [](uint64_t lane, uint64_t word, uint64_t k) {
		const uint64_t m = (lane ^ word) * k;
		return (m << 29) | (m >> 35);
	};
	size_t i = 0;
	uint64_t h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3];  // (written out: the loop every noted byte goes through)
	for (; i + 32 <= bytes; i += 32) {
		uint64_t w[4];
		__builtin_memcpy(w, p + i, 32);
		h0 = (h0 ^ w[0]) * K[0];
		h1 = (h1 ^ w[1]) * K[1];
		h2 = (h2 ^ w[2]) * K[2];
		h3 = (h3 ^ w[3]) * K[3];
		h0 = (h0 << 29) | (h0 >> 35);
		h1 = (h1 << 29) | (h1 >> 35);
		h2 = (h2 << 29) | (h2 >> 35);
		h3 = (h3 << 29) | (h3 >> 35);
	}
	h[0] = h0, h[1] = h1, h[2] = h2, h[3] = h3;
	for (int lane = 0; i + 8 <= bytes; i += 8, ++lane) {
		uint64_t w;
		__builtin_memcpy(&w, p + i, 8);
		h[lane] = step(h[lane], w, K[lane]);
	}
	if (i < bytes) {  // (4 bytes are left: an odd number of floats, or of 12-byte triplets)
		uint32_t w;
		__builtin_memcpy(&w, p + i, 4);
		h[3] = step(h[3], 0x100000000ull | w, K[3]);
	}
}

inline uint64_t mix_lanes(uint64_t f, const uint64_t h[4])
{
	for (int lane = 0; lane < 4; ++lane) {
		f = (f ^ h[lane]) * 0xFF51AFD7ED558CCDull;
		f ^= f >> 32;
	}
	return f;
}

// of the triplets [a, b) and the right-hand sides of the rows [r0, r1): every one of them, in their order, and the two counts
inline uint64_t range_checksum(const std::vector<Triplet>& t, size_t a, size_t b, const std::vector<float>& rhs, size_t r0, size_t r1)
{
	static_assert(sizeof(float) == 4 && sizeof(Triplet) == 12, "triplets and right-hand sides are read as packed 4-byte fields");
	uint64_t ht[4] = {1469598103934665603ull, static_cast<uint64_t>(b - a), 0x2545F4914F6CDD1Dull, 0};
	uint64_t hr[4] = {static_cast<uint64_t>(r1 - r0), 0x9FB21C651E98DF25ull, 0, 0x27D4EB2F165667C5ull};
	if (b > a) { mix_bytes(ht, reinterpret_cast<const unsigned char*>(t.data() + a), (b - a) * sizeof(Triplet)); }
	if (r1 > r0) { mix_bytes(hr, reinterpret_cast<const unsigned char*>(rhs.data() + r0), (r1 - r0) * sizeof(float)); }
	return mix_lanes(mix_lanes(0, ht), hr);
}

// Whether eq's note still describes eq: there is one, it is for this lattice (`lattice` null or empty: whatever lattice the
// note names) of one to three dimensions, its ranges lie in order inside eq.triplets and eq.rhs, every triplet and every
// right-hand side in them is the one that was noted, and at most one range holds model rows.  What lies outside the noted
// ranges -- rows the caller appended -- is not looked at.  The solvers (RowsOnGpu::from_recipe) ask this at every solve.
inline bool noted_rows_unchanged(const LinearEquation& eq, const std::vector<int>* lattice)
{
	const Recipe* r = eq.recipe.get();
	if (!r || r->segments.empty()) { return false; }
	if (lattice && !lattice->empty() && *lattice != r->sizes) { return false; }
	if (r->sizes.empty() || r->sizes.size() > 3) { return false; }
	bool   model = false;
	size_t row_end = 0, trip_end = 0;
	for (const Segment& s : r->segments) {
		if (s.row0 < row_end || s.trip0 < trip_end || s.row1 < s.row0 || s.trip1 < s.trip0 || s.row1 > eq.rhs.size() ||
		    s.trip1 > eq.triplets.size()) {
			return false;
		}
		row_end  = s.row1;
		trip_end = s.trip1;
		if (range_checksum(eq.triplets, s.trip0, s.trip1, eq.rhs, s.row0, s.row1) != s.checksum) { return false; }
		if (s.kind == Segment::kModel) {
			if (model) { return false; }
			model = true;
		}
	}
	return true;
}

}  // namespace detail
}  // namespace field_interpolation
