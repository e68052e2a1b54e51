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
// Structure and query: fi_bvh.h's tree and stackless walk over the usable primitives, sorted by the Morton code of their box
// centres, their vertex coordinates stored inline in sorted order, leaves of kSurfLeaf consecutive primitives; this file
// supplies the primitives as items and their distance.  Exactness (fi_bvh.h has the argument): c lies inside its
// primitive's vertex box by the clamp, hence inside every enclosing node box.
#include "fi_solver_internal.h"
#include "fi_surface.h"
#include "fi_dual.h"
#include "fi_bvh.h"

#include <memory>

namespace fi {

namespace {

using namespace bvh;

constexpr int kSurfLeaf = 8;

// the items of the build (fi_bvh.h): np primitives of D vertex indices into nv vertices of D floats; usable means every
// vertex finite, an index outside [0, nv) is counted as bad; stored as 3-D: three float4 (a, b, c; the primitive's index as
// bits in the first .w), 2-D: one float4 (ax, ay, bx, by) and the index in ids
template <int D>
struct PrimItems {
	static constexpr int  kDim = D, kLeaf = kSurfLeaf, kVerts = D, kSlots = D == 3 ? 3 : 1, kBoxAxes = D;
	static constexpr bool kIds = D == 2;
	int64_t nv;
	const float* __restrict__ pos;
	const int* __restrict__ idx;
	// vertex k at v[k * D]; with a bad index nothing is read
	__device__ int load(int64_t i, float* v) const
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
	// the centre of the vertex box
	__device__ void key_point(const float* v, double* m) const
	{
#pragma unroll
		for (int d = 0; d < D; ++d) {
			float l = v[d], h = v[d];
#pragma unroll
			for (int k = 1; k < D; ++k) {
				l = fminf(l, v[k * D + d]);
				h = fmaxf(h, v[k * D + d]);
			}
			m[d] = 0.5 * (static_cast<double>(l) + static_cast<double>(h));
		}
	}
	__device__ void store(int64_t i, uint32_t j, const float* v, float4* __restrict__ prims, uint32_t* __restrict__ ids) const
	{
		if constexpr (D == 3) {
			prims[3 * i]     = make_float4(v[0], v[1], v[2], __uint_as_float(j));
			prims[3 * i + 1] = make_float4(v[3], v[4], v[5], 0.0f);
			prims[3 * i + 2] = make_float4(v[6], v[7], v[8], 0.0f);
		} else {
			prims[i] = make_float4(v[0], v[1], v[2], v[3]);
			ids[i]   = j;
		}
	}
	__device__ static void extend(const float4* __restrict__ prims, int64_t i, float4& lo, float4& hi)
	{
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
	void check(const uint32_t* c, int64_t np) const
	{
		FI_REQUIRE(c[1] == 0, FI_ERR_INVALID, "%u primitives index a vertex outside [0, %lld)", c[1], static_cast<long long>(nv));
		FI_REQUIRE(c[0] <= static_cast<uint64_t>(np), FI_ERR_HIP, "surface: %u usable primitives of %lld", c[0], static_cast<long long>(np));
	}
};

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

// where the queries come from, and what is written
enum { kFromBuffer = 0, kFromLattice = 1, kRedistance = 2 };

struct QueryArgs {
	Tree         t;
	int64_t      n;
	const float* q;         // kFromBuffer: float[n][D]
	Lattice      l;         // kFromLattice / kRedistance: the lattice and its tiles
	const float* field;     // kRedistance: the fp32 field whose sign is applied
	float        iso;
	int          dual;      // kRedistance: inside is f - iso <= 0 (else f < iso)
	float        lim;       // the largest float whose sqrtf is <= max_distance
	float*       dist;
	long long*   idx;       // or nullptr
	float*       closest;   // kFromBuffer: float[n][D] or nullptr
};

// 7 waves per SIMD: the 3-D test keeps Ericson's six dot products and both the edge and the face candidates live at once
// (70 VGPRs; asking for 8 waves spills 8-10 of them); 2-D needs 32-36
template <int D, int SRC>
__global__ __launch_bounds__(kThreads, 7) void k_surf_query(QueryArgs a)
{
	float   q[D];
	int64_t out;
	if constexpr (SRC == kFromBuffer) {
		out = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
		if (out >= a.n) { return; }
#pragma unroll
		for (int d = 0; d < D; ++d) { q[d] = a.q[out * D + d]; }
	} else {
		if (!lattice_query<D>(a.l, q, &out)) { return; }
	}
	const bool finite = finite_point<D>(q);
	float      best   = NAN;
	uint32_t   bidx   = kNone;  // the smallest primitive index that reaches best, and its place in the sorted set
	int64_t    slot   = -1;
	if (finite) {
		search<D, kSurfLeaf>(a.t, q, a.lim, best, [&](int64_t i, float& least) {
			float       c[D];
			uint32_t    j = 0;
			const float s = primitive_point<D>(a.t.items, i, q, c, &j);
			if (s <= least) {  // (false for a NaN)
				if constexpr (D == 2) { j = a.t.ids[i]; }
				if (s < least || j < bidx) {
					least = s;
					bidx  = j;
					slot  = i;
				}
			}
		});
	}
	float dist = distance_of(finite, best, a.lim, bidx);
	if constexpr (SRC == kRedistance) {
		const float f      = a.field[out];
		const bool  inside = a.dual ? f - a.iso <= 0.0f : f < a.iso;
		dist = inside ? -dist : dist;
	}
	a.dist[out] = dist;
	if (a.idx) { a.idx[out] = index_of(bidx); }
	if constexpr (SRC == kFromBuffer) {
		if (a.closest) {
			float c[D];
			if (bidx != kNone) {
				uint32_t j = 0;
				(void)primitive_point<D>(a.t.items, slot, q, c, &j);  // the same arithmetic: the same bits
			} else {
#pragma unroll
				for (int d = 0; d < D; ++d) { c[d] = NAN; }
			}
#pragma unroll
			for (int d = 0; d < D; ++d) { a.closest[out * D + d] = c[d]; }
		}
	}
}

template <int SRC>
void launch_query(int D, dim3 grid, const QueryArgs& a, hipStream_t st)
{
	if (D == 2) {
		hipLaunchKernelGGL((k_surf_query<2, SRC>), grid, dim3(kThreads), 0, st, a);
	} else {
		hipLaunchKernelGGL((k_surf_query<3, SRC>), grid, dim3(kThreads), 0, st, a);
	}
	FI_HIP_TRY(hipGetLastError());
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
		build(t, PrimItems<2>{nv, vertices, indices}, np, st);
	} else {
		build(t, PrimItems<3>{nv, vertices, indices}, np, st);
	}
}

void surface_query(const SurfaceIndex& t, int64_t n, const float* queries, float max_distance, float* distances, long long* primitives,
                   float* closest, int memory, hipStream_t st)
{
	if (n == 0) { return; }
	AllocStream alloc_on(st);
	Outputs o(n, t.D, distances, primitives, closest, memory);
	stage::In<float> q(queries, n * t.D, memory, st);
	QueryArgs a{};
	a.t       = tree_of(t);
	a.n       = n;
	a.q       = q;
	a.lim     = limit_for(max_distance);
	a.dist    = o.dist;
	a.idx     = o.idx;
	a.closest = o.cl;
	launch_query<kFromBuffer>(t.D, dim3(blocks_for(n)), a, st);
	o.finish(st);
}

void surface_lattice(const SurfaceIndex& t, const int* sizes, float max_distance, float* out, long long* primitives, int memory,
                     hipStream_t st)
{
	QueryArgs     a{};
	int64_t       total = 0;
	const dim3    grid  = lattice_grid(t.D, sizes, a.l, &total);
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
	const dim3 grid  = lattice_grid(ndim, sizes, a.l, &total);
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
	const float* f = field_f32(c, field, memory, buf);  // (an fp64 solution is rounded once: the sign comes from the same field as the mesh)
	redistance_whole(f, g.ndim, g.gn, iso, method, max_distance, out, primitives, mesh, memory, c->stream);
}

}  // namespace fi
