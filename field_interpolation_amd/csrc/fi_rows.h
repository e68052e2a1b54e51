// fi_rows.h -- the rows of ONE data point: its value row and its D gradient rows as "cell rows" (extended cell id, 2^D
// corner coefficients, rhs), with the reference's fp32 arithmetic in the reference's order (multilerp,
// field_interpolation.cpp:15-55).  One device function for everybody who needs them: k_emit_rows (fi_assembly.hip) writes
// them to the row tables, k_point_residual (fi_robust.hip) applies them to a field.  Every translation unit that includes
// this header is compiled with -ffp-contract=off: one rounding per operation.
#pragma once

#include "fi_internal.h"

namespace fi {

struct EmitArgs {
	Geom  g;
	float vw, gw;
	int   vk, gk;
	int   has_nrm, has_pw, has_val;
	int   rows_per_point;        // 1 + D, or 1 when the batch has no gradient rows (no normals or a zero gradient weight)
	uint32_t invalid_key;
	float pos_scale, nrm_scale;  // 1 on the caller's lattice; 1/2^l and 2^l on coarser levels
};

// Extended local cell id of the cell with GLOBAL origin c[] (origins run from -1), or invalid when the
// cell does not touch this rank's slab.
template <int D>
__device__ inline uint32_t cell_key(const Geom& g, const int* c, uint32_t invalid)
{
	uint32_t key = 0;
	uint32_t mul = 1;
	for (int d = 0; d < D; ++d) {
		const int l = c[d] - g.coff[d];
		if (l < 0 || l >= g.cn[d]) { return invalid; }
		key += static_cast<uint32_t>(l) * mul;
		mul *= static_cast<uint32_t>(g.cn[d]);
	}
	return key;
}

// The rows of point i, handed one after another to sink.row(r, key, origin, c, b): r = 0 the value row, r = 1 + d the
// gradient row along d (only when the batch has gradient rows); key = a.invalid_key for a row the point does not emit
// (outside the lattice, non-finite, a zero weight), else the row's cell, whose GLOBAL origin is origin[0 .. D-1]; c[q] the
// coefficient of corner q (bit d of q: +1 along axis d), b the right-hand side.
// w multiplies into the coefficients; gate decides whether a row exists at all (gate * weight != 0).  The assembly passes
// the point's weight for both; the residual pass measures at w = 1 the rows the point's weight admits.
template <int D, typename Sink>
__device__ inline void point_rows(const EmitArgs& a, long i, const float* __restrict__ pos, const float* __restrict__ nrm,
                                  float w, float gate, float value, Sink& sink)
{
	constexpr int NC = 1 << D;
	const Geom& g = a.g;

	float p[D];
	bool  finite = true;
	for (int d = 0; d < D; ++d) {
		p[d]   = pos[i * D + d] * a.pos_scale;
		if (g.pshift[d] != 0.0f) { p[d] += g.pshift[d]; }  // a level halved cell-centred along d
		finite = finite && isfinite(p[d]);
	}

	// cell of the point: floor(pos) per axis (multilerp :29-32, cell_index :115)
	int   cell[D];
	float t[D];
	bool  cell_in_ext = finite;  // origin within [-1, size-1] on every axis
	bool  cell_valid  = finite;  // 0 <= origin and origin + 1 < size (cell_index :116)
	for (int d = 0; d < D; ++d) {
		const float fl = floorf(p[d]);
		if (!(fl >= -1.0f && fl <= static_cast<float>(g.gn[d] - 1))) {
			cell_in_ext = false;
			cell_valid  = false;
			cell[d]     = 0;
			t[d]        = 0.0f;
			continue;
		}
		cell[d] = static_cast<int>(fl);
		t[d]    = p[d] - static_cast<float>(cell[d]);
		if (!(0 <= cell[d] && cell[d] + 1 < g.gn[d])) { cell_valid = false; }
	}

	// ---- value row ----------------------------------------------------------------------------
	{
		const float cw = w * a.vw;
		const bool  on = gate * a.vw != 0.0f;
		uint32_t k = a.invalid_key;
		float    c[NC];
		float    b = 0.0f;
		int      origin[D];
		for (int d = 0; d < D; ++d) { origin[d] = cell[d]; }
		for (int q = 0; q < NC; ++q) { c[q] = 0.0f; }
		if (a.vk == FI_VALUE_LINEAR_INTERPOLATION) {
			// field_interpolation.cpp:57-80: corners outside the lattice are dropped, the kept weights
			// are not renormalised; rhs = (sum of kept coefficient) * value.
			if (on && cell_in_ext) {
				int   kept = 0;
				float sum  = 0.0f;
				for (int q = 0; q < NC; ++q) {
					float lw = 1.0f;
					bool  in = true;
					for (int d = 0; d < D; ++d) {
						const int up = (q >> d) & 1;
						const int cc = cell[d] + up;
						lw *= up ? t[d] : 1.0f - t[d];
						in = in && (0 <= cc) && (cc < g.gn[d]);
					}
					if (in) {
						const float s = lw * cw;
						c[q] = s;
						sum += s;
						++kept;
					}
				}
				if (kept > 0) {
					k = cell_key<D>(g, cell, a.invalid_key);
					b = sum * value;
				}
			}
		} else {
			// field_interpolation.cpp:82-107 through add_equation (sparse_linear.cpp:34-50): nearest
			// lattice point by std::round; row [1]*cw, rhs (value - (pos-nearest).gradient)*cw.
			if (on && finite) {
				bool  ok    = true;
				float along = 0.0f;
				int   corner = 0;
				int   cc[D];
				for (int d = 0; d < D; ++d) {
					const float r = roundf(p[d]);
					if (!(r >= 0.0f && r <= static_cast<float>(g.gn[d] - 1))) {
						ok = false;
						cc[d] = 0;
						continue;
					}
					const int q = static_cast<int>(r);
					along += (p[d] - static_cast<float>(q)) * (nrm[i * D + d] * a.nrm_scale);
					// the nearest point is a corner of the (extended) cell floor(pos)
					int base = static_cast<int>(floorf(p[d]));
					if (base < -1) { base = -1; }
					if (base > q) { base = q; }
					if (q - base > 1) { base = q - 1; }
					cc[d] = base;
					corner |= (q - base) << d;
				}
				if (ok) {
					k = cell_key<D>(g, cc, a.invalid_key);
					c[corner] = 1.0f * cw;
					b = (value - along) * cw;
					for (int d = 0; d < D; ++d) { origin[d] = cc[d]; }
				}
			}
		}
		sink.row(0, k, origin, c, b);
	}

	// ---- gradient rows ------------------------------------------------------------------------
	if (a.rows_per_point == 1) { return; }
	for (int d = 0; d < D; ++d) {
		uint32_t k = a.invalid_key;
		float    c[NC];
		float    b = 0.0f;
		for (int q = 0; q < NC; ++q) { c[q] = 0.0f; }
		if (a.has_nrm) {
			const float cw = w * a.gw;
			const bool  on = gate * a.gw != 0.0f;
			const float gd = nrm[i * D + d] * a.nrm_scale;
			if (on && cell_valid) {
				if (a.gk == FI_GRADIENT_NEAREST_NEIGHBOR) {
					// field_interpolation.cpp:134-149: [-1, +1]*cw on the cell edge along d.
					c[0]      = -1.0f * cw;
					c[1 << d] = +1.0f * cw;
					b         = gd * cw;
					k         = cell_key<D>(g, cell, a.invalid_key);
				} else if (a.gk == FI_GRADIENT_CELL_EDGES) {
					// field_interpolation.cpp:150-187: +-cw*2/2^D on all corners, rhs cw*g_d.
					const float term = cw * 2.0f / static_cast<float>(NC);
					for (int q = 0; q < NC; ++q) { c[q] = (((q >> d) & 1) ? +1.0f : -1.0f) * term; }
					b = cw * gd;
					k = cell_key<D>(g, cell, a.invalid_key);
				}
			}
		}
		sink.row(1 + d, k, cell, c, b);
	}
}

}  // namespace fi
