// fi_surface.hip -- exact distances to a segment (2-D) or triangle (3-D) mesh on the device, and the redistancing of a
// lattice field against its own iso-surface.
//
// The contract (include/fi_hip.h fi_surface_distance): the closest point c(q, prim) of a segment is its
// clamped projection, of a triangle Ericson's ClosestPtPointTriangle (Real-Time Collision Detection 5.1.5) with its
// Voronoi-region tests in its order; a triangle whose chosen branch divides by a denominator that is not > 0 is degenerate
// and gives the nearest of its three edges' segment points.  c is then clamped per axis into the primitive's vertex box.
// s = 0.0f + (q_0 - c_0)^2 + ... in ascending axes, fp32 with one rounding per operation (-ffp-contract=off); the result
// is sqrtf of the minimum s and the smallest primitive index that reaches it.
//
// Structure (fi_nearest.hip's, over primitives): the usable primitives sorted by the Morton code of their box centres
// (rocPRIM radix sort), their vertex coordinates stored inline in sorted order, leaves of kSurfLeaf consecutive primitives
// and an implicit balanced binary tree over them whose node boxes come from a level-by-level min / max reduction.
//
// Query: one thread per query, the stackless depth-first walk of fi_nearest.hip (near child first, a node pruned only when
// lb > best).  Exactness: c lies inside its primitive's vertex box by the clamp, hence inside every enclosing node box, and
// lb is formed like s from the per-axis gaps to the box; rounding is monotone, so lb <= s holds bit for bit.
#include "fi_solver_internal.h"
#include "fi_surface.h"
#include "fi_dual.h"
#include "fi_prim.h"

#include <cmath>
#include <memory>

namespace fi {

namespace {

constexpr int      kSurfLeaf     = 8;
constexpr int      kSurfThreads  = 256;
constexpr int      kBoundsBlocks = 256;
constexpr uint32_t kNone         = 0xFFFFFFFFu;

// float4 slots per stored primitive
__host__ __device__ constexpr int slots(int D) { return D == 3 ? 3 : 1; }

// Morton bits per axis and the key of an unusable primitive (sorted behind every usable one)
__host__ __device__ constexpr int morton_bits(int D) { return D == 3 ? 21 : 24; }
__host__ __device__ constexpr uint64_t unusable_key(int D) { return uint64_t(1) << (D * morton_bits(D)); }

__device__ inline uint64_t spread(uint32_t v, int D)
{
	uint64_t x = v;
	if (D == 2) {
		x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
		x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
		x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
		x = (x | (x << 2)) & 0x3333333333333333ull;
		x = (x | (x << 1)) & 0x5555555555555555ull;
		return x;
	}
	x = (x | (x << 32)) & 0x1F00000000FFFFull;
	x = (x | (x << 16)) & 0x1F0000FF0000FFull;
	x = (x | (x << 8)) & 0x100F00F00F00F00Full;
	x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
	x = (x | (x << 2)) & 0x1249249249249249ull;
	return x;
}

// the vertices of primitive i into v[D * D] (vertex k at v[k * D]); 0: usable, 1: a non-finite coordinate, 2: an index
// outside [0, nv) (nothing read)
template <int D>
__device__ inline int load_primitive(int64_t i, int64_t nv, const float* __restrict__ pos, const int* __restrict__ idx, float* v)
{
	int64_t j[D];
#pragma unroll
	for (int k = 0; k < D; ++k) {
		j[k] = idx[i * D + k];
		if (j[k] < 0 || j[k] >= nv) { return 2; }
	}
	bool ok = true;
#pragma unroll
	for (int k = 0; k < D; ++k) {
#pragma unroll
		for (int d = 0; d < D; ++d) {
			v[k * D + d] = pos[j[k] * D + d];
			ok = ok && isfinite(v[k * D + d]);
		}
	}
	return ok ? 0 : 1;
}

// bounds of the usable primitives' vertices: per-block partials (lo[3], hi[3], usable count, bad-index count) ...
template <int D>
__global__ __launch_bounds__(kSurfThreads) void k_surf_bounds(int64_t np, int64_t nv, const float* __restrict__ pos,
                                                              const int* __restrict__ idx, float* __restrict__ part,
                                                              uint32_t* __restrict__ cnt)
{
	__shared__ float    s_lo[3][kSurfThreads], s_hi[3][kSurfThreads];
	__shared__ uint32_t s_n[2][kSurfThreads];
	float    lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
	uint32_t m = 0, bad = 0;
	for (int64_t i = static_cast<int64_t>(blockIdx.x) * kSurfThreads + threadIdx.x; i < np;
	     i += static_cast<int64_t>(gridDim.x) * kSurfThreads) {
		float     v[D * D];
		const int r = load_primitive<D>(i, nv, pos, idx, v);
		bad += r == 2 ? 1u : 0u;
		if (r != 0) { continue; }
		++m;
#pragma unroll
		for (int k = 0; k < D; ++k) {
#pragma unroll
			for (int d = 0; d < D; ++d) {
				lo[d] = fminf(lo[d], v[k * D + d]);
				hi[d] = fmaxf(hi[d], v[k * D + d]);
			}
		}
	}
	const int t = threadIdx.x;
	for (int d = 0; d < 3; ++d) {
		s_lo[d][t] = lo[d];
		s_hi[d][t] = hi[d];
	}
	s_n[0][t] = m;
	s_n[1][t] = bad;
	__syncthreads();
	for (int w = kSurfThreads / 2; w > 0; w >>= 1) {
		if (t < w) {
			for (int d = 0; d < 3; ++d) {
				s_lo[d][t] = fminf(s_lo[d][t], s_lo[d][t + w]);
				s_hi[d][t] = fmaxf(s_hi[d][t], s_hi[d][t + w]);
			}
			s_n[0][t] += s_n[0][t + w];
			s_n[1][t] += s_n[1][t + w];
		}
		__syncthreads();
	}
	if (t == 0) {
		for (int d = 0; d < 3; ++d) {
			part[blockIdx.x * 6 + d]     = s_lo[d][0];
			part[blockIdx.x * 6 + 3 + d] = s_hi[d][0];
		}
		cnt[2 * blockIdx.x]     = s_n[0][0];
		cnt[2 * blockIdx.x + 1] = s_n[1][0];
	}
}

// ... and their reduction by one block: bounds part[6 kBoundsBlocks ..), the counts cnt[2 kBoundsBlocks], cnt[2 kBoundsBlocks + 1]
__global__ __launch_bounds__(kBoundsBlocks) void k_surf_bounds_total(float* __restrict__ part, uint32_t* __restrict__ cnt)
{
	__shared__ float    s_b[6][kBoundsBlocks];
	__shared__ uint32_t s_n[2][kBoundsBlocks];
	const int t = threadIdx.x;
	for (int e = 0; e < 6; ++e) { s_b[e][t] = part[t * 6 + e]; }
	s_n[0][t] = cnt[2 * t];
	s_n[1][t] = cnt[2 * t + 1];
	__syncthreads();
	for (int w = kBoundsBlocks / 2; w > 0; w >>= 1) {
		if (t < w) {
			for (int e = 0; e < 3; ++e) {
				s_b[e][t]     = fminf(s_b[e][t], s_b[e][t + w]);
				s_b[3 + e][t] = fmaxf(s_b[3 + e][t], s_b[3 + e][t + w]);
			}
			s_n[0][t] += s_n[0][t + w];
			s_n[1][t] += s_n[1][t + w];
		}
		__syncthreads();
	}
	if (t == 0) {
		for (int e = 0; e < 6; ++e) { part[kBoundsBlocks * 6 + e] = s_b[e][0]; }
		cnt[2 * kBoundsBlocks]     = s_n[0][0];
		cnt[2 * kBoundsBlocks + 1] = s_n[1][0];
	}
}

template <int D>
__global__ __launch_bounds__(kSurfThreads) void k_surf_morton(int64_t np, int64_t nv, const float* __restrict__ pos,
                                                              const int* __restrict__ idx, const float* __restrict__ bounds,
                                                              uint64_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kSurfThreads + threadIdx.x;
	if (i >= np) { return; }
	float    v[D * D];
	uint64_t key = unusable_key(D);
	if (load_primitive<D>(i, nv, pos, idx, v) == 0) {
		constexpr double top = static_cast<double>((1u << morton_bits(D)) - 1u);
		key = 0;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			float l = v[d], h = v[d];
#pragma unroll
			for (int k = 1; k < D; ++k) {
				l = fminf(l, v[k * D + d]);
				h = fmaxf(h, v[k * D + d]);
			}
			const double lo = bounds[d], ext = static_cast<double>(bounds[3 + d]) - lo;
			const double mid = 0.5 * (static_cast<double>(l) + static_cast<double>(h));
			const double u   = ext > 0.0 ? (mid - lo) * (top / ext) : 0.0;
			const uint32_t b = static_cast<uint32_t>(fmin(fmax(u, 0.0), top));
			key |= spread(b, D) << d;
		}
	}
	keys[i] = key;
	vals[i] = static_cast<uint32_t>(i);
}

// the usable primitives in sorted order, vertices inline
template <int D>
__global__ __launch_bounds__(kSurfThreads) void k_surf_gather(int64_t nf, int64_t nv, const float* __restrict__ pos,
                                                              const int* __restrict__ idx, const uint32_t* __restrict__ order,
                                                              float4* __restrict__ prims, uint32_t* __restrict__ ids)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kSurfThreads + threadIdx.x;
	if (i >= nf) { return; }
	const uint32_t j = order[i];
	float          v[D * D];
	(void)load_primitive<D>(j, nv, pos, idx, v);  // (usable: sorted before every unusable one)
	if constexpr (D == 3) {
		prims[3 * i]     = make_float4(v[0], v[1], v[2], __uint_as_float(j));
		prims[3 * i + 1] = make_float4(v[3], v[4], v[5], 0.0f);
		prims[3 * i + 2] = make_float4(v[6], v[7], v[8], 0.0f);
	} else {
		prims[i] = make_float4(v[0], v[1], v[2], v[3]);
		ids[i]   = j;
	}
}

// the boxes of the leaves (node P + j; an empty leaf gets lo = +inf > hi = -inf) ...
template <int D>
__global__ __launch_bounds__(kSurfThreads) void k_surf_leaves(int64_t nf, int64_t P, const float4* __restrict__ prims,
                                                              float4* __restrict__ box)
{
	const int64_t j = static_cast<int64_t>(blockIdx.x) * kSurfThreads + threadIdx.x;
	if (j >= P) { return; }
	float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.0f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
	const int64_t b = j * kSurfLeaf, e = b + kSurfLeaf < nf ? b + kSurfLeaf : nf;
	for (int64_t i = b; i < e; ++i) {
		if constexpr (D == 3) {
			for (int k = 0; k < 3; ++k) {
				const float4 p = prims[3 * i + k];
				lo.x = fminf(lo.x, p.x), lo.y = fminf(lo.y, p.y), lo.z = fminf(lo.z, p.z);
				hi.x = fmaxf(hi.x, p.x), hi.y = fmaxf(hi.y, p.y), hi.z = fmaxf(hi.z, p.z);
			}
		} else {
			const float4 p = prims[i];
			lo.x = fminf(lo.x, fminf(p.x, p.z)), lo.y = fminf(lo.y, fminf(p.y, p.w));
			hi.x = fmaxf(hi.x, fmaxf(p.x, p.z)), hi.y = fmaxf(hi.y, fmaxf(p.y, p.w));
		}
	}
	if constexpr (D == 2) { lo.z = hi.z = 0.0f; }
	box[2 * (P + j)]     = lo;
	box[2 * (P + j) + 1] = hi;
}

// ... and of the nodes [first, 2 first) of one level from their children
__global__ __launch_bounds__(kSurfThreads) void k_surf_nodes(int64_t first, float4* __restrict__ box)
{
	const int64_t k = first + static_cast<int64_t>(blockIdx.x) * kSurfThreads + threadIdx.x;
	if (k >= 2 * first) { return; }
	const float4 l0 = box[4 * k], h0 = box[4 * k + 1], l1 = box[4 * k + 2], h1 = box[4 * k + 3];
	box[2 * k]     = make_float4(fminf(l0.x, l1.x), fminf(l0.y, l1.y), fminf(l0.z, l1.z), 0.0f);
	box[2 * k + 1] = make_float4(fmaxf(h0.x, h1.x), fmaxf(h0.y, h1.y), fmaxf(h0.z, h1.z), 0.0f);
}

// ---- the closest point: the contract's arithmetic ----------------------------------------------------------------------

// dot products sum in ascending axes from the first term
template <int D>
__device__ inline float dot(const float* u, const float* v)
{
	float s = u[0] * v[0];
#pragma unroll
	for (int d = 1; d < D; ++d) { s = s + u[d] * v[d]; }
	return s;
}

// the segment's point before the box clamp: t = dot(q - a, ab) / dot(ab, ab) (0 when that is not > 0), clamped to [0, 1]
template <int D>
__device__ inline void segment_point(const float* q, const float* a, const float* b, float* c)
{
	float ab[D], aq[D];
#pragma unroll
	for (int d = 0; d < D; ++d) {
		ab[d] = b[d] - a[d];
		aq[d] = q[d] - a[d];
	}
	const float den = dot<D>(ab, ab);
	float       t   = den > 0.0f ? dot<D>(aq, ab) / den : 0.0f;
	t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
#pragma unroll
	for (int d = 0; d < D; ++d) { c[d] = a[d] + t * ab[d]; }
}

template <int D>
__device__ inline float sq_dist(const float* q, const float* c)
{
	float s = 0.0f;
#pragma unroll
	for (int d = 0; d < D; ++d) {
		const float e = q[d] - c[d];
		s = s + e * e;
	}
	return s;
}

// the nearest of the three edges' segment points, in edge order ab, bc, ca, the first on ties
__device__ inline void degenerate_point(const float* q, const float* a, const float* b, const float* c, float* out)
{
	float p[3], r[3];
	segment_point<3>(q, a, b, out);
	float best = sq_dist<3>(q, out);
	segment_point<3>(q, b, c, p);
	float s = sq_dist<3>(q, p);
	segment_point<3>(q, c, a, r);
	const float s2   = sq_dist<3>(q, r);
	const bool  take = s < best;
	best = take ? s : best;
#pragma unroll
	for (int d = 0; d < 3; ++d) { out[d] = take ? p[d] : out[d]; }
	const bool take2 = s2 < best;
#pragma unroll
	for (int d = 0; d < 3; ++d) { out[d] = take2 ? r[d] : out[d]; }
}

// Ericson's ClosestPtPointTriangle: the branches become selects (the rounding of each candidate is the branch's own), with one
// quotient for whichever edge region applies; a degenerate branch (its denominator not > 0) takes the three-edge rule
__device__ inline void triangle_point(const float* p, const float* a, const float* b, const float* c, float* out)
{
	float ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		ab[d] = b[d] - a[d];
		ac[d] = c[d] - a[d];
		ap[d] = p[d] - a[d];
		bp[d] = p[d] - b[d];
		cp[d] = p[d] - c[d];
	}
	const float d1 = dot<3>(ab, ap), d2 = dot<3>(ac, ap);
	const float d3 = dot<3>(ab, bp), d4 = dot<3>(ac, bp);
	const float d5 = dot<3>(ab, cp), d6 = dot<3>(ac, cp);
	const float vc = d1 * d4 - d3 * d2;
	const float vb = d5 * d2 - d1 * d6;
	const float va = d3 * d6 - d5 * d4;
	const float e43 = d4 - d3, e56 = d5 - d6;
	const bool rA  = d1 <= 0.0f && d2 <= 0.0f;
	const bool rB  = d3 >= 0.0f && d4 <= d3;
	const bool rAB = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
	const bool rC  = d6 >= 0.0f && d5 <= d6;
	const bool rAC = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
	const bool rBC = va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f;
	// the first region in Ericson's order: 0 A, 1 B, 2 AB, 3 C, 4 AC, 5 BC, 6 the face
	const int r = rA ? 0 : rB ? 1 : rAB ? 2 : rC ? 3 : rAC ? 4 : rBC ? 5 : 6;
	// the edge regions: base + (num / den) * dir
	const bool  onA = r != 5;
	const float num = r == 2 ? d1 : (r == 4 ? d2 : e43);
	const float den = r == 2 ? d1 - d3 : (r == 4 ? d2 - d6 : e43 + e56);
	const float t   = num / den;
	// the face: a + ab v + ac w, v = vb / sum, w = vc / sum through one reciprocal
	const float sum = (va + vb) + vc;
	const float inv = 1.0f / sum;
	const float v = vb * inv, w = vc * inv;
	const bool  edge = r == 2 || r == 4 || r == 5;
	if ((edge && !(den > 0.0f)) || (r == 6 && !(sum > 0.0f))) {
		degenerate_point(p, a, b, c, out);
		return;
	}
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		const float dir = r == 2 ? ab[d] : (r == 4 ? ac[d] : c[d] - b[d]);
		const float ep  = (onA ? a[d] : b[d]) + t * dir;
		const float fp  = (a[d] + ab[d] * v) + ac[d] * w;
		out[d] = r == 0 ? a[d] : r == 1 ? b[d] : r == 3 ? c[d] : edge ? ep : fp;
	}
}

// c(q, primitive i of the sorted set) clamped into its vertex box, and s
template <int D>
__device__ inline float primitive_point(const float4* __restrict__ prims, int64_t i, const float* q, float* c, uint32_t* j)
{
	float lo[D], hi[D];
	if constexpr (D == 3) {
		const float4 r0 = prims[3 * i], r1 = prims[3 * i + 1], r2 = prims[3 * i + 2];
		const float  a[3] = {r0.x, r0.y, r0.z}, b[3] = {r1.x, r1.y, r1.z}, cc[3] = {r2.x, r2.y, r2.z};
		*j = __float_as_uint(r0.w);
		triangle_point(q, a, b, cc, c);
#pragma unroll
		for (int d = 0; d < 3; ++d) {
			lo[d] = fminf(fminf(a[d], b[d]), cc[d]);
			hi[d] = fmaxf(fmaxf(a[d], b[d]), cc[d]);
		}
	} else {
		const float4 r = prims[i];
		const float  a[2] = {r.x, r.y}, b[2] = {r.z, r.w};
		segment_point<2>(q, a, b, c);
#pragma unroll
		for (int d = 0; d < 2; ++d) {
			lo[d] = fminf(a[d], b[d]);
			hi[d] = fmaxf(a[d], b[d]);
		}
	}
#pragma unroll
	for (int d = 0; d < D; ++d) { c[d] = c[d] < lo[d] ? lo[d] : (c[d] > hi[d] ? hi[d] : c[d]); }
	return sq_dist<D>(q, c);
}

struct Tree {
	const float4*   prims;
	const uint32_t* ids;   // 2-D: the primitives' indices
	const float4*   box;
	int64_t         nf;
	uint32_t        P;
	int             H;
};

// lb of node k, or false for an empty node
template <int D>
__device__ inline bool node_lb(const Tree& t, uint32_t k, const float* q, float* lb)
{
	const float4 lo4 = t.box[2 * k], hi4 = t.box[2 * k + 1];
	if (!(lo4.x <= hi4.x)) { return false; }
	const float lo[3] = {lo4.x, lo4.y, lo4.z}, hi[3] = {hi4.x, hi4.y, hi4.z};
	float       s = 0.0f;
#pragma unroll
	for (int d = 0; d < D; ++d) {
		const float g = q[d] < lo[d] ? lo[d] - q[d] : (q[d] > hi[d] ? q[d] - hi[d] : 0.0f);
		s = s + g * g;
	}
	*lb = s;
	return true;
}

// the search of one finite query: best = min s (+inf if none), bidx = its smallest index (kNone if none), slot = its place
// in the sorted set; lim: prune nodes with lb > lim as well (sqrtf(lb) > max_distance)
template <int D>
__device__ void search(const Tree& t, const float* q, float lim, float& best, uint32_t& bidx, int64_t& slot)
{
	best = INFINITY;
	bidx = kNone;
	slot = -1;
	if (t.nf == 0) { return; }
	float lb;
	if (!node_lb<D>(t, 1, q, &lb) || lb > lim) { return; }
	uint32_t k = 1, second = 0;
	int      depth = 0;
	for (;;) {
		// node k is admitted: visit it
		if (depth == t.H) {
			const int64_t b = static_cast<int64_t>(k - t.P) * kSurfLeaf;
			const int64_t e = b + kSurfLeaf < t.nf ? b + kSurfLeaf : t.nf;
			for (int64_t i = b; i < e; ++i) {
				float     c[D];
				uint32_t  j = 0;
				const float s = primitive_point<D>(t.prims, i, q, c, &j);
				if (s <= best) {  // (false for a NaN)
					if constexpr (D == 2) { j = t.ids[i]; }
					if (s < best || j < bidx) {
						best = s;
						bidx = j;
						slot = i;
					}
				}
			}
		} else {
			const float cut = fminf(best, lim);
			float       l0 = 0.0f, l1 = 0.0f;
			const bool  a0 = node_lb<D>(t, 2 * k, q, &l0) && l0 <= cut;
			const bool  a1 = node_lb<D>(t, 2 * k + 1, q, &l1) && l1 <= cut;
			if (a0 || a1) {
				k = 2 * k + ((a1 && (!a0 || l1 < l0)) ? 1u : 0u);  // the near child first (a tie: the left one)
				++depth;
				continue;
			}
		}
		// node k is done: the sibling of the first child of each level, if it is still worth a look, else up
		for (;;) {
			if (depth == 0) { return; }
			const uint32_t bit = 1u << (depth - 1);
			if (!(second & bit)) {
				second |= bit;
				const float cut = fminf(best, lim);
				if (node_lb<D>(t, k ^ 1u, q, &lb) && lb <= cut) {
					k ^= 1u;
					break;
				}
			}
			second &= ~bit;
			k >>= 1;
			--depth;
		}
	}
}

// where the queries come from, and what is written
enum { kFromBuffer = 0, kFromLattice = 1, kRedistance = 2 };

struct QueryArgs {
	Tree         t;
	int64_t      n;
	const float* q;         // kFromBuffer: float[n][D]
	int          sz[3];     // kFromLattice / kRedistance: the lattice
	int64_t      tiles[3];  // tiles per axis
	const float* field;     // kRedistance: the fp32 field whose sign is applied
	float        iso;
	int          dual;      // kRedistance: inside is f - iso <= 0 (else f < iso)
	float        lim;       // the largest float whose sqrtf is <= max_distance
	float*       dist;
	long long*   idx;       // or nullptr
	float*       closest;   // kFromBuffer: float[n][D] or nullptr
};

// the tile of kSurfThreads lattice points a block walks (x fastest): fi_nearest.hip's, coherent queries in a workgroup
template <int D>
struct TileShape;
template <>
struct TileShape<2> { static constexpr int e[3] = {16, 16, 1}; };
template <>
struct TileShape<3> { static constexpr int e[3] = {8, 8, 4}; };

// 7 waves per SIMD: the 3-D test keeps Ericson's six dot products and both the edge and the face candidates live at once
// (70 VGPRs; asking for 8 waves spills 8-10 of them); 2-D needs 32-36
template <int D, int SRC>
__global__ __launch_bounds__(kSurfThreads, 7) void k_surf_query(QueryArgs a)
{
	float   q[D];
	int64_t out;
	if constexpr (SRC == kFromBuffer) {
		out = static_cast<int64_t>(blockIdx.x) * kSurfThreads + threadIdx.x;
		if (out >= a.n) { return; }
#pragma unroll
		for (int d = 0; d < D; ++d) { q[d] = a.q[out * D + d]; }
	} else {
		int64_t b = blockIdx.x;
		int     c[3];
		int     tid = threadIdx.x;
		bool    in  = true;
#pragma unroll
		for (int d = 0; d < 3; ++d) {
			const int64_t tc = b % a.tiles[d];
			b /= a.tiles[d];
			c[d] = static_cast<int>(tc) * TileShape<D>::e[d] + tid % TileShape<D>::e[d];
			tid /= TileShape<D>::e[d];
			in   = in && c[d] < a.sz[d];
		}
		if (!in) { return; }
		out = c[0] + static_cast<int64_t>(a.sz[0]) * (c[1] + static_cast<int64_t>(a.sz[1]) * c[2]);
#pragma unroll
		for (int d = 0; d < D; ++d) { q[d] = static_cast<float>(c[d]); }
	}
	bool finite = true;
#pragma unroll
	for (int d = 0; d < D; ++d) { finite = finite && isfinite(q[d]); }
	float    best = NAN;
	uint32_t bidx = kNone;
	int64_t  slot = -1;
	if (finite) { search<D>(a.t, q, a.lim, best, bidx, slot); }
	float dist = best;  // (NaN for a non-finite query)
	if (finite) {
		if (bidx != kNone && best > a.lim) { bidx = kNone; }  // beyond max_distance
		dist = bidx == kNone ? INFINITY : sqrtf(best);
	}
	if constexpr (SRC == kRedistance) {
		const float f      = a.field[out];
		const bool  inside = a.dual ? f - a.iso <= 0.0f : f < a.iso;
		dist = inside ? -dist : dist;
	}
	a.dist[out] = dist;
	if (a.idx) { a.idx[out] = bidx == kNone ? -1LL : static_cast<long long>(bidx); }
	if constexpr (SRC == kFromBuffer) {
		if (a.closest) {
			float c[D];
			if (bidx != kNone) {
				uint32_t j = 0;
				(void)primitive_point<D>(a.t.prims, slot, q, c, &j);  // the same arithmetic: the same bits
			} else {
#pragma unroll
				for (int d = 0; d < D; ++d) { c[d] = NAN; }
			}
#pragma unroll
			for (int d = 0; d < D; ++d) { a.closest[out * D + d] = c[d]; }
		}
	}
}

Tree tree_of(const SurfaceIndex& t)
{
	return Tree{t.prims.as<float4>(), t.ids.as<uint32_t>(), t.box.as<float4>(), t.nf, static_cast<uint32_t>(uint32_t(1) << t.H), t.H};
}

// sqrtf(lb) > max_distance  <=>  lb > lim: the largest float whose (correctly rounded) square root is <= max_distance
float limit_for(float max_distance)
{
	if (std::isinf(max_distance)) { return INFINITY; }
	const double sq = static_cast<double>(max_distance) * max_distance;
	float        x  = sq > 3.4e38 ? INFINITY : static_cast<float>(sq);
	while (x > 0.0f && std::sqrt(x) > max_distance) { x = std::nextafter(x, 0.0f); }
	while (std::sqrt(std::nextafter(x, INFINITY)) <= max_distance) { x = std::nextafter(x, INFINITY); }
	return x;
}

template <int SRC>
void launch_query(int D, dim3 grid, const QueryArgs& a, hipStream_t st)
{
	if (D == 2) {
		hipLaunchKernelGGL((k_surf_query<2, SRC>), grid, dim3(kSurfThreads), 0, st, a);
	} else {
		hipLaunchKernelGGL((k_surf_query<3, SRC>), grid, dim3(kSurfThreads), 0, st, a);
	}
	FI_HIP_TRY(hipGetLastError());
}

dim3 query_blocks(int64_t n) { return dim3(static_cast<unsigned>((n + kSurfThreads - 1) / kSurfThreads)); }

// the lattice's tiles; the grid of blocks
dim3 lattice_grid(int D, const int* sizes, QueryArgs& a, int64_t* total)
{
	int64_t blocks = 1;
	*total = 1;
	for (int d = 0; d < 3; ++d) {
		const int e = D == 2 ? TileShape<2>::e[d] : TileShape<3>::e[d];
		a.sz[d]     = d < D ? sizes[d] : 1;
		a.tiles[d]  = (a.sz[d] + e - 1) / e;
		*total *= a.sz[d];
		blocks *= a.tiles[d];
	}
	FI_REQUIRE(*total < (int64_t(1) << 31), FI_ERR_UNSUPPORTED, "a lattice of %lld points", static_cast<long long>(*total));
	return dim3(static_cast<unsigned>(blocks));
}

// outputs of a call on the device: the caller's (FI_DEVICE) or staged (FI_HOST), copied back by finish()
struct Outputs {
	int64_t    n;
	int        D, memory;
	float*     dist;
	long long* idx;
	float*     cl;
	float*     host_dist;
	long long* host_idx;
	float*     host_cl;
	DevBuf     bd, bi, bc;
	Outputs(int64_t count, int ndim, float* distances, long long* indices, float* closest, int mem)
	    : n(count), D(ndim), memory(mem), dist(distances), idx(indices), cl(closest), host_dist(distances), host_idx(indices),
	      host_cl(closest)
	{
		if (memory == FI_DEVICE) { return; }
		bd.alloc(sizeof(float) * n);
		dist = bd.as<float>();
		if (indices) {
			bi.alloc(sizeof(long long) * n);
			idx = bi.as<long long>();
		}
		if (closest) {
			bc.alloc(sizeof(float) * D * n);
			cl = bc.as<float>();
		}
	}
	void finish(hipStream_t st)
	{
		if (memory == FI_HOST) {
			FI_HIP_TRY(hipMemcpyAsync(host_dist, dist, sizeof(float) * n, hipMemcpyDeviceToHost, st));
			if (idx) { FI_HIP_TRY(hipMemcpyAsync(host_idx, idx, sizeof(long long) * n, hipMemcpyDeviceToHost, st)); }
			if (cl) { FI_HIP_TRY(hipMemcpyAsync(host_cl, cl, sizeof(float) * D * n, hipMemcpyDeviceToHost, st)); }
		}
		FI_HIP_TRY(hipStreamSynchronize(st));
	}
};

template <int D>
void build_kernels(SurfaceIndex& t, int64_t nv, const float* pos, int64_t np, const int* idx, hipStream_t st)
{
	DevBuf part, cnt, keys, keys2, vals, vals2, tmp;
	part.alloc(sizeof(float) * 6 * (kBoundsBlocks + 1));
	cnt.alloc(sizeof(uint32_t) * 2 * (kBoundsBlocks + 1));
	hipLaunchKernelGGL(k_surf_bounds<D>, dim3(kBoundsBlocks), dim3(kSurfThreads), 0, st, np, nv, pos, idx, part.as<float>(),
	                   cnt.as<uint32_t>());
	hipLaunchKernelGGL(k_surf_bounds_total, dim3(1), dim3(kBoundsBlocks), 0, st, part.as<float>(), cnt.as<uint32_t>());
	keys.alloc(sizeof(uint64_t) * np);
	keys2.alloc(sizeof(uint64_t) * np);
	vals.alloc(sizeof(uint32_t) * np);
	vals2.alloc(sizeof(uint32_t) * np);
	hipLaunchKernelGGL(k_surf_morton<D>, query_blocks(np), dim3(kSurfThreads), 0, st, np, nv, pos, idx,
	                   part.as<float>() + 6 * kBoundsBlocks, keys.as<uint64_t>(), vals.as<uint32_t>());
	FI_HIP_TRY(hipGetLastError());
	const int end_bit = D * morton_bits(D) + 1;
	size_t    tb      = 0;
	FI_HIP_TRY(prim::sort_pairs_u64(nullptr, tb, keys.as<uint64_t>(), keys2.as<uint64_t>(), vals.as<uint32_t>(), vals2.as<uint32_t>(),
	                                static_cast<size_t>(np), 0, end_bit, st));
	tmp.alloc(tb);
	FI_HIP_TRY(prim::sort_pairs_u64(tmp.p, tb, keys.as<uint64_t>(), keys2.as<uint64_t>(), vals.as<uint32_t>(), vals2.as<uint32_t>(),
	                                static_cast<size_t>(np), 0, end_bit, st));
	uint32_t c[2] = {0, 0};
	FI_HIP_TRY(hipMemcpyAsync(c, cnt.as<uint32_t>() + 2 * kBoundsBlocks, sizeof(c), hipMemcpyDeviceToHost, st));
	FI_HIP_TRY(hipStreamSynchronize(st));
	FI_REQUIRE(c[1] == 0, FI_ERR_INVALID, "%u primitives index a vertex outside [0, %lld)", c[1], static_cast<long long>(nv));
	FI_REQUIRE(c[0] <= static_cast<uint64_t>(np), FI_ERR_HIP, "surface: %u usable primitives of %lld", c[0], static_cast<long long>(np));
	t.nf = c[0];
	if (t.nf == 0) { return; }
	const int64_t leaves = (t.nf + kSurfLeaf - 1) / kSurfLeaf;
	while ((int64_t(1) << t.H) < leaves) { ++t.H; }
	const int64_t P = int64_t(1) << t.H;
	t.prims.alloc(sizeof(float4) * slots(D) * t.nf);
	if (D == 2) { t.ids.alloc(sizeof(uint32_t) * t.nf); }
	t.box.alloc(sizeof(float4) * 4 * P);
	hipLaunchKernelGGL(k_surf_gather<D>, query_blocks(t.nf), dim3(kSurfThreads), 0, st, t.nf, nv, pos, idx, vals2.as<uint32_t>(),
	                   t.prims.as<float4>(), t.ids.as<uint32_t>());
	hipLaunchKernelGGL(k_surf_leaves<D>, query_blocks(P), dim3(kSurfThreads), 0, st, t.nf, P, t.prims.as<float4>(), t.box.as<float4>());
	for (int64_t first = P / 2; first >= 1; first /= 2) {
		hipLaunchKernelGGL(k_surf_nodes, query_blocks(first), dim3(kSurfThreads), 0, st, first, t.box.as<float4>());
	}
	FI_HIP_TRY(hipGetLastError());
	FI_HIP_TRY(hipStreamSynchronize(st));  // the temporaries die here
}

}  // namespace

void surface_build(SurfaceIndex& t, int ndim, int64_t nv, const float* vertices, int64_t np, const int* indices, hipStream_t st)
{
	FI_REQUIRE(ndim == 2 || ndim == 3, FI_ERR_UNSUPPORTED, "surfaces of %d-D lattices are not supported (2-D segments, 3-D triangles)",
	           ndim);
	FI_REQUIRE(np < (int64_t(1) << 31), FI_ERR_UNSUPPORTED, "%lld primitives: primitive indices are 32-bit", static_cast<long long>(np));
	t.D  = ndim;
	t.np = np;
	t.nf = 0;
	t.H  = 0;
	if (np == 0) { return; }
	if (ndim == 2) {
		build_kernels<2>(t, nv, vertices, np, indices, st);
	} else {
		build_kernels<3>(t, nv, vertices, np, indices, st);
	}
}

void surface_query(const SurfaceIndex& t, int64_t n, const float* queries, float max_distance, float* distances, long long* primitives,
                   float* closest, int memory, hipStream_t st)
{
	if (n == 0) { return; }
	AllocStream alloc_on(st);
	Outputs o(n, t.D, distances, primitives, closest, memory);
	DevBuf  bq;
	const float* q = queries;
	if (memory == FI_HOST) {
		bq.alloc(sizeof(float) * t.D * n);
		FI_HIP_TRY(hipMemcpyAsync(bq.p, queries, sizeof(float) * t.D * n, hipMemcpyHostToDevice, st));
		q = bq.as<float>();
	}
	QueryArgs a{};
	a.t       = tree_of(t);
	a.n       = n;
	a.q       = q;
	a.lim     = limit_for(max_distance);
	a.dist    = o.dist;
	a.idx     = o.idx;
	a.closest = o.cl;
	launch_query<kFromBuffer>(t.D, query_blocks(n), a, st);
	o.finish(st);
}

void surface_lattice(const SurfaceIndex& t, const int* sizes, float max_distance, float* out, long long* primitives, int memory,
                     hipStream_t st)
{
	QueryArgs     a{};
	int64_t       total = 0;
	const dim3    grid  = lattice_grid(t.D, sizes, a, &total);
	AllocStream   alloc_on(st);
	Outputs       o(total, t.D, out, primitives, nullptr, memory);
	a.t    = tree_of(t);
	a.n    = total;
	a.lim  = limit_for(max_distance);
	a.dist = o.dist;
	a.idx  = o.idx;
	launch_query<kFromLattice>(t.D, grid, a, st);
	o.finish(st);
}

void redistance_whole(const float* field, int ndim, const int* sizes, float iso, int method, float max_distance, float* out,
                      long long* primitives, fi_mesh** mesh, int memory, hipStream_t st)
{
	FI_REQUIRE(method == FI_SURFACE_ISO || method == FI_SURFACE_DUAL, FI_ERR_INVALID, "unknown surface method %d", method);
	AllocStream alloc_on(st);
	fi_mesh*    m = nullptr;
	if (method == FI_SURFACE_ISO) {
		iso_extract_whole(field, ndim, sizes, iso, 1, nullptr, nullptr, st, &m);
	} else {
		dual_contour_whole(field, nullptr, ndim, sizes, iso, st, &m);
	}
	std::unique_ptr<fi_mesh> own(m);
	SurfaceIndex t;
	surface_build(t, ndim, own->nv, own->pos.as<float>(), own->np, own->idx.as<int>(), st);
	QueryArgs  a{};
	int64_t    total = 0;
	const dim3 grid  = lattice_grid(ndim, sizes, a, &total);
	Outputs    o(total, ndim, out, primitives, nullptr, memory);
	a.t     = tree_of(t);
	a.n     = total;
	a.field = field;
	a.iso   = iso;
	a.dual  = method == FI_SURFACE_DUAL ? 1 : 0;
	a.lim   = limit_for(max_distance);
	a.dist  = o.dist;
	a.idx   = o.idx;
	launch_query<kRedistance>(ndim, grid, a, st);
	o.finish(st);
	if (mesh) { *mesh = own.release(); }
}

void redistance_ctx(fi_ctx* c, const float* field, float iso, int method, float max_distance, float* out, long long* primitives,
                    fi_mesh** mesh, int memory)
{
	const Geom& g = c->g;
	FI_REQUIRE(c->nranks == 1, FI_ERR_UNSUPPORTED,
	           "redistancing a slab context: a rank holds only part of the surface (a primitive exchange is not implemented)");
	FI_REQUIRE(g.ndim == 2 || g.ndim == 3, FI_ERR_UNSUPPORTED, "redistancing a %d-D lattice is not supported", g.ndim);
	FI_REQUIRE(field || c->vectors_ready, FI_ERR_STATE, "no solution yet");
	AllocStream alloc_on(c->stream);
	DevBuf       buf;
	const float* f = nullptr;
	if (field && memory == FI_DEVICE) {
		f = field;
	} else if (field) {
		buf.alloc(sizeof(float) * g.nown);
		FI_HIP_TRY(hipMemcpyAsync(buf.p, field, sizeof(float) * g.nown, hipMemcpyHostToDevice, c->stream));
		f = buf.as<float>();
	} else if (c->dtype == FI_F32) {
		f = owned<float>(c, c->x);
	} else {  // an fp64 solution, rounded to fp32 once, as fi_iso_extract does: the sign comes from the same field as the mesh
		buf.alloc(sizeof(float) * g.nown);
		hipLaunchKernelGGL((k_to_float<double>), dim3(blocks_for(g.nown)), dim3(kThreads), 0, c->stream, g.nown,
		                   owned<double>(c, c->x), buf.as<float>());
		FI_HIP_TRY(hipGetLastError());
		f = buf.as<float>();
	}
	redistance_whole(f, g.ndim, g.gn, iso, method, max_distance, out, primitives, mesh, memory, c->stream);
}

}  // namespace fi
