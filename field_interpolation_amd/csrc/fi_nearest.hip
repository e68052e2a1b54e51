// fi_nearest.hip -- exact nearest data points on the device.
//
// The contract (include/fi_hip.h fi_nearest): s(p, q) is the fp32 sum from 0.0f of (p_d - q_d)^2 in ascending
// d, one rounding per operation (-ffp-contract=off) -- the arithmetic of the reference's border-prior loop; the result of a
// query is sqrtf of the minimum of s over the finite points and the smallest index that reaches it.
//
// Structure: the finite points sorted by a Morton code over their own bounding box (rocPRIM radix sort), leaves of
// kNearestLeaf consecutive points and an implicit balanced binary tree over them (heap numbering, 2^H leaves, empty ones at
// the end).  Node boxes come from a level-by-level min / max reduction: no atomics, the same tree on every run.
//
// Query: one thread per query, depth first, the near child first, a node pruned only when its lower bound lb > best (strict:
// an equal s in another leaf may still carry a smaller index).  lb is formed like s from the per-axis gaps lo - q / q - hi;
// rounding is monotone, so lb <= s holds bit for bit for every point of the box and no margin is needed.  The walk keeps no
// stack: a node's children are 2k and 2k + 1, so going up is k >> 1 and the sibling is k ^ 1, and one bit per level says
// whether the sibling has been looked at yet -- two registers instead of a stack indexed at run time (which would spill).
#include "fi_solver_internal.h"
#include "fi_nearest.h"
#include "fi_prim.h"

#include <cmath>

namespace fi {

namespace {

constexpr int      kNearestLeaf    = 16;
constexpr int      kNearestThreads = 256;
constexpr int      kBoundsBlocks   = 256;
constexpr uint32_t kNone           = 0xFFFFFFFFu;

// Morton bits per axis and the key of a non-finite point (sorted behind every finite one)
__host__ __device__ constexpr int morton_bits(int D) { return D == 3 ? 21 : 24; }
__host__ __device__ constexpr uint64_t nonfinite_key(int D) { return uint64_t(1) << (D * morton_bits(D)); }

__device__ inline uint64_t spread(uint32_t v, int D)
{
	if (D == 1) { return v; }
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

template <int D>
__device__ inline bool finite_point(const float* p)
{
	bool ok = true;
#pragma unroll
	for (int d = 0; d < D; ++d) { ok = ok && isfinite(p[d]); }
	return ok;
}

// bounds of the finite points: per-block partials (lo[3], hi[3], count) ...
template <int D>
__global__ __launch_bounds__(kNearestThreads) void k_nearest_bounds(int64_t n, const float* __restrict__ pos, float* __restrict__ part,
                                                                     uint32_t* __restrict__ cnt)
{
	__shared__ float    s_lo[3][kNearestThreads], s_hi[3][kNearestThreads];
	__shared__ uint32_t s_n[kNearestThreads];
	float    lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
	uint32_t m = 0;
	for (int64_t i = static_cast<int64_t>(blockIdx.x) * kNearestThreads + threadIdx.x; i < n;
	     i += static_cast<int64_t>(gridDim.x) * kNearestThreads) {
		float p[D];
#pragma unroll
		for (int d = 0; d < D; ++d) { p[d] = pos[i * D + d]; }
		if (!finite_point<D>(p)) { continue; }
		++m;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			lo[d] = fminf(lo[d], p[d]);
			hi[d] = fmaxf(hi[d], p[d]);
		}
	}
	const int t = threadIdx.x;
	for (int d = 0; d < 3; ++d) {
		s_lo[d][t] = lo[d];
		s_hi[d][t] = hi[d];
	}
	s_n[t] = m;
	__syncthreads();
	for (int w = kNearestThreads / 2; w > 0; w >>= 1) {
		if (t < w) {
			for (int d = 0; d < 3; ++d) {
				s_lo[d][t] = fminf(s_lo[d][t], s_lo[d][t + w]);
				s_hi[d][t] = fmaxf(s_hi[d][t], s_hi[d][t + w]);
			}
			s_n[t] += s_n[t + w];
		}
		__syncthreads();
	}
	if (t == 0) {
		for (int d = 0; d < 3; ++d) {
			part[blockIdx.x * 6 + d]     = s_lo[d][0];
			part[blockIdx.x * 6 + 3 + d] = s_hi[d][0];
		}
		cnt[blockIdx.x] = s_n[0];
	}
}

// ... and their reduction by one block: bounds[0 .. 6) and the count of finite points in cnt[kBoundsBlocks]
__global__ __launch_bounds__(kBoundsBlocks) void k_nearest_bounds_total(float* __restrict__ part, uint32_t* __restrict__ cnt)
{
	__shared__ float    s_b[6][kBoundsBlocks];
	__shared__ uint32_t s_n[kBoundsBlocks];
	const int t = threadIdx.x;
	for (int e = 0; e < 6; ++e) { s_b[e][t] = part[t * 6 + e]; }
	s_n[t] = cnt[t];
	__syncthreads();
	for (int w = kBoundsBlocks / 2; w > 0; w >>= 1) {
		if (t < w) {
			for (int e = 0; e < 3; ++e) {
				s_b[e][t]     = fminf(s_b[e][t], s_b[e][t + w]);
				s_b[3 + e][t] = fmaxf(s_b[3 + e][t], s_b[3 + e][t + w]);
			}
			s_n[t] += s_n[t + w];
		}
		__syncthreads();
	}
	if (t == 0) {
		for (int e = 0; e < 6; ++e) { part[kBoundsBlocks * 6 + e] = s_b[e][0]; }
		cnt[kBoundsBlocks] = s_n[0];
	}
}

template <int D>
__global__ __launch_bounds__(kNearestThreads) void k_nearest_morton(int64_t n, const float* __restrict__ pos, const float* __restrict__ bounds,
                                                                     uint64_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kNearestThreads + threadIdx.x;
	if (i >= n) { return; }
	float p[D];
#pragma unroll
	for (int d = 0; d < D; ++d) { p[d] = pos[i * D + d]; }
	uint64_t key = nonfinite_key(D);
	if (finite_point<D>(p)) {
		constexpr double top = static_cast<double>((1u << morton_bits(D)) - 1u);
		key = 0;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			const double lo = bounds[d], ext = static_cast<double>(bounds[3 + d]) - lo;
			const double u  = ext > 0.0 ? (static_cast<double>(p[d]) - lo) * (top / ext) : 0.0;
			const uint32_t b = static_cast<uint32_t>(fmin(fmax(u, 0.0), top));
			key |= spread(b, D) << d;
		}
	}
	keys[i] = key;
	vals[i] = static_cast<uint32_t>(i);
}

template <int D>
__global__ __launch_bounds__(kNearestThreads) void k_nearest_gather(int64_t nf, const float* __restrict__ pos, const uint32_t* __restrict__ order,
                                                                     float4* __restrict__ pts)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kNearestThreads + threadIdx.x;
	if (i >= nf) { return; }
	const uint32_t j = order[i];
	float          p[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
	for (int d = 0; d < D; ++d) { p[d] = pos[static_cast<int64_t>(j) * D + d]; }
	pts[i] = make_float4(p[0], p[1], p[2], __uint_as_float(j));
}

// the boxes of the leaves (node P + j; an empty leaf gets lo = +inf > hi = -inf) ...
__global__ __launch_bounds__(kNearestThreads) void k_nearest_leaves(int64_t nf, int64_t P, const float4* __restrict__ pts, float4* __restrict__ box)
{
	const int64_t j = static_cast<int64_t>(blockIdx.x) * kNearestThreads + threadIdx.x;
	if (j >= P) { return; }
	float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.0f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
	const int64_t b = j * kNearestLeaf, e = b + kNearestLeaf < nf ? b + kNearestLeaf : nf;
	for (int64_t i = b; i < e; ++i) {
		const float4 p = pts[i];
		lo.x = fminf(lo.x, p.x), lo.y = fminf(lo.y, p.y), lo.z = fminf(lo.z, p.z);
		hi.x = fmaxf(hi.x, p.x), hi.y = fmaxf(hi.y, p.y), hi.z = fmaxf(hi.z, p.z);
	}
	box[2 * (P + j)]     = lo;
	box[2 * (P + j) + 1] = hi;
}

// ... and of the nodes [first, 2 first) of one level from their children
__global__ __launch_bounds__(kNearestThreads) void k_nearest_nodes(int64_t first, float4* __restrict__ box)
{
	const int64_t k = first + static_cast<int64_t>(blockIdx.x) * kNearestThreads + threadIdx.x;
	if (k >= 2 * first) { return; }
	const float4 l0 = box[4 * k], h0 = box[4 * k + 1], l1 = box[4 * k + 2], h1 = box[4 * k + 3];
	box[2 * k]     = make_float4(fminf(l0.x, l1.x), fminf(l0.y, l1.y), fminf(l0.z, l1.z), 0.0f);
	box[2 * k + 1] = make_float4(fmaxf(h0.x, h1.x), fmaxf(h0.y, h1.y), fmaxf(h0.z, h1.z), 0.0f);
}

struct Tree {
	const float4* pts;
	const float4* box;
	int64_t       nf;
	uint32_t      P;
	int           H;
};

template <int D>
__device__ inline float sq_dist(const float4& p, const float* q)
{
	const float c[3] = {p.x, p.y, p.z};
	float       s    = 0.0f;
#pragma unroll
	for (int d = 0; d < D; ++d) {
		const float e = c[d] - q[d];
		s = s + e * e;
	}
	return s;
}

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

// the search of one finite query: best = min s (+inf if none), bidx = its smallest index (kNone if none); lim: prune nodes
// with lb > lim as well (sqrtf(lb) > max_distance)
template <int D>
__device__ void search(const Tree& t, const float* q, float lim, float& best, uint32_t& bidx)
{
	best = INFINITY;
	bidx = kNone;
	if (t.nf == 0) { return; }
	float lb;
	if (!node_lb<D>(t, 1, q, &lb) || lb > lim) { return; }
	uint32_t k = 1, second = 0;
	int      depth = 0;
	for (;;) {
		// node k is admitted: visit it
		if (depth == t.H) {
			const int64_t b = static_cast<int64_t>(k - t.P) * kNearestLeaf;
			const int64_t e = b + kNearestLeaf < t.nf ? b + kNearestLeaf : t.nf;
			for (int64_t i = b; i < e; ++i) {
				const float4   p = t.pts[i];
				const float    s = sq_dist<D>(p, q);
				const uint32_t j = __float_as_uint(p.w);
				if (s < best || (s == best && j < bidx)) {
					best = s;
					bidx = j;
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

// where the queries come from
enum { kFromBuffer = 0, kFromLattice = 1, kFromList = 2 };

struct QueryArgs {
	Tree             t;
	int64_t          n;
	const float*     q;        // kFromBuffer: float[n][D]
	int              sz[3];    // kFromLattice / kFromList: the lattice
	int64_t          tiles[3]; // kFromLattice: tiles per axis
	const uint32_t*  list;     // kFromList: linear lattice indices
	float            lim;      // the largest float whose sqrtf is <= max_distance
	float*           dist;
	long long*       idx;      // or nullptr
	float*           d2;       // kFromList: the squared distance
};

// the tile of kNearestThreads lattice points a block walks (x fastest): coherent queries in a workgroup
template <int D>
struct TileShape;
template <>
struct TileShape<1> { static constexpr int e[3] = {256, 1, 1}; };
template <>
struct TileShape<2> { static constexpr int e[3] = {16, 16, 1}; };
template <>
struct TileShape<3> { static constexpr int e[3] = {8, 8, 4}; };

template <int D, int SRC>
__global__ __launch_bounds__(kNearestThreads) void k_nearest_query(QueryArgs a)
{
	float   q[D];
	int64_t out;
	if constexpr (SRC == kFromLattice) {
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
	} else {
		out = static_cast<int64_t>(blockIdx.x) * kNearestThreads + threadIdx.x;
		if (out >= a.n) { return; }
		if constexpr (SRC == kFromList) {
			uint32_t r = a.list[out];
#pragma unroll
			for (int d = 0; d < D; ++d) {
				q[d] = static_cast<float>(r % static_cast<uint32_t>(a.sz[d]));
				r /= static_cast<uint32_t>(a.sz[d]);
			}
		} else {
#pragma unroll
			for (int d = 0; d < D; ++d) { q[d] = a.q[out * D + d]; }
		}
	}
	bool finite = true;
#pragma unroll
	for (int d = 0; d < D; ++d) { finite = finite && isfinite(q[d]); }
	float    best = NAN;
	uint32_t bidx = kNone;
	if (finite) { search<D>(a.t, q, a.lim, best, bidx); }
	if constexpr (SRC == kFromList) {
		a.d2[out] = best;
		return;
	}
	float dist = best;  // (NaN for a non-finite query)
	if (finite) {
		if (bidx != kNone && best > a.lim) { bidx = kNone; }  // beyond max_distance
		// (a finite point whose s overflows is still the nearest: +inf with its index)
		dist = bidx == kNone ? INFINITY : sqrtf(best);
	}
	a.dist[out] = dist;
	if (a.idx) { a.idx[out] = bidx == kNone ? -1LL : static_cast<long long>(bidx); }
}

Tree tree_of(const NearestIndex& t)
{
	return Tree{t.pts.as<float4>(), t.box.as<float4>(), t.nf, static_cast<uint32_t>(uint32_t(1) << t.H), t.H};
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
	switch (D) {
	case 1: hipLaunchKernelGGL((k_nearest_query<1, SRC>), grid, dim3(kNearestThreads), 0, st, a); break;
	case 2: hipLaunchKernelGGL((k_nearest_query<2, SRC>), grid, dim3(kNearestThreads), 0, st, a); break;
	default: hipLaunchKernelGGL((k_nearest_query<3, SRC>), grid, dim3(kNearestThreads), 0, st, a); break;
	}
	FI_HIP_TRY(hipGetLastError());
}

dim3 query_blocks(int64_t n) { return dim3(static_cast<unsigned>((n + kNearestThreads - 1) / kNearestThreads)); }

// outputs of a call on the device: the caller's (FI_DEVICE) or staged (FI_HOST), copied back by finish()
struct Outputs {
	int64_t    n;
	int        memory;
	float*     dist;
	long long* idx;
	float*     host_dist;
	long long* host_idx;
	DevBuf     bd, bi;
	Outputs(int64_t count, float* distances, long long* indices, int mem)
	    : n(count), memory(mem), dist(distances), idx(indices), host_dist(distances), host_idx(indices)
	{
		if (memory == FI_DEVICE) { return; }
		bd.alloc(sizeof(float) * n);
		dist = bd.as<float>();
		if (indices) {
			bi.alloc(sizeof(long long) * n);
			idx = bi.as<long long>();
		}
	}
	void finish(hipStream_t st)
	{
		if (memory == FI_HOST) {
			FI_HIP_TRY(hipMemcpyAsync(host_dist, dist, sizeof(float) * n, hipMemcpyDeviceToHost, st));
			if (idx) { FI_HIP_TRY(hipMemcpyAsync(host_idx, idx, sizeof(long long) * n, hipMemcpyDeviceToHost, st)); }
		}
		FI_HIP_TRY(hipStreamSynchronize(st));
	}
};

}  // namespace

void nearest_build(NearestIndex& t, int D, int64_t n, const float* const* seg_pos, const int64_t* seg_n, int nseg, hipStream_t st)
{
	t.D  = D;
	t.n  = n;
	t.nf = 0;
	t.H  = 0;
	if (n == 0) { return; }
	FI_REQUIRE(n < (int64_t(1) << 31), FI_ERR_UNSUPPORTED, "%lld points: nearest-point indices are 32-bit", static_cast<long long>(n));
	DevBuf all, part, cnt, keys, keys2, vals, vals2, tmp;
	const float* pos = seg_pos[0];
	if (nseg > 1) {  // one contiguous set
		all.alloc(sizeof(float) * D * n);
		int64_t at = 0;
		for (int s = 0; s < nseg; ++s) {
			if (seg_n[s] > 0) {
				FI_HIP_TRY(hipMemcpyAsync(all.as<float>() + at * D, seg_pos[s], sizeof(float) * D * seg_n[s], hipMemcpyDeviceToDevice, st));
			}
			at += seg_n[s];
		}
		pos = all.as<float>();
	}
	part.alloc(sizeof(float) * 6 * (kBoundsBlocks + 1));
	cnt.alloc(sizeof(uint32_t) * (kBoundsBlocks + 1));
	const dim3 grid = query_blocks(n);
	switch (D) {
	case 1:
		hipLaunchKernelGGL(k_nearest_bounds<1>, dim3(kBoundsBlocks), dim3(kNearestThreads), 0, st, n, pos, part.as<float>(), cnt.as<uint32_t>());
		break;
	case 2:
		hipLaunchKernelGGL(k_nearest_bounds<2>, dim3(kBoundsBlocks), dim3(kNearestThreads), 0, st, n, pos, part.as<float>(), cnt.as<uint32_t>());
		break;
	default:
		hipLaunchKernelGGL(k_nearest_bounds<3>, dim3(kBoundsBlocks), dim3(kNearestThreads), 0, st, n, pos, part.as<float>(), cnt.as<uint32_t>());
		break;
	}
	hipLaunchKernelGGL(k_nearest_bounds_total, dim3(1), dim3(kBoundsBlocks), 0, st, part.as<float>(), cnt.as<uint32_t>());
	keys.alloc(sizeof(uint64_t) * n);
	keys2.alloc(sizeof(uint64_t) * n);
	vals.alloc(sizeof(uint32_t) * n);
	vals2.alloc(sizeof(uint32_t) * n);
	const float* bounds = part.as<float>() + 6 * kBoundsBlocks;
	switch (D) {
	case 1: hipLaunchKernelGGL(k_nearest_morton<1>, grid, dim3(kNearestThreads), 0, st, n, pos, bounds, keys.as<uint64_t>(), vals.as<uint32_t>()); break;
	case 2: hipLaunchKernelGGL(k_nearest_morton<2>, grid, dim3(kNearestThreads), 0, st, n, pos, bounds, keys.as<uint64_t>(), vals.as<uint32_t>()); break;
	default: hipLaunchKernelGGL(k_nearest_morton<3>, grid, dim3(kNearestThreads), 0, st, n, pos, bounds, keys.as<uint64_t>(), vals.as<uint32_t>()); break;
	}
	FI_HIP_TRY(hipGetLastError());
	const int end_bit = D * morton_bits(D) + 1;
	size_t    tb      = 0;
	FI_HIP_TRY(prim::sort_pairs_u64(nullptr, tb, keys.as<uint64_t>(), keys2.as<uint64_t>(), vals.as<uint32_t>(), vals2.as<uint32_t>(),
	                                static_cast<size_t>(n), 0, end_bit, st));
	tmp.alloc(tb);
	FI_HIP_TRY(prim::sort_pairs_u64(tmp.p, tb, keys.as<uint64_t>(), keys2.as<uint64_t>(), vals.as<uint32_t>(), vals2.as<uint32_t>(),
	                                static_cast<size_t>(n), 0, end_bit, st));
	uint32_t nf = 0;
	FI_HIP_TRY(hipMemcpyAsync(&nf, cnt.as<uint32_t>() + kBoundsBlocks, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	FI_HIP_TRY(hipStreamSynchronize(st));
	FI_REQUIRE(nf <= static_cast<uint64_t>(n), FI_ERR_HIP, "nearest: %u finite points of %lld", nf, static_cast<long long>(n));
	t.nf = nf;
	if (nf == 0) { return; }
	const int64_t leaves = (static_cast<int64_t>(nf) + kNearestLeaf - 1) / kNearestLeaf;
	while ((int64_t(1) << t.H) < leaves) { ++t.H; }
	const int64_t P = int64_t(1) << t.H;
	t.pts.alloc(sizeof(float4) * nf);
	t.box.alloc(sizeof(float4) * 4 * P);
	switch (D) {
	case 1: hipLaunchKernelGGL(k_nearest_gather<1>, query_blocks(nf), dim3(kNearestThreads), 0, st, static_cast<int64_t>(nf), pos, vals2.as<uint32_t>(), t.pts.as<float4>()); break;
	case 2: hipLaunchKernelGGL(k_nearest_gather<2>, query_blocks(nf), dim3(kNearestThreads), 0, st, static_cast<int64_t>(nf), pos, vals2.as<uint32_t>(), t.pts.as<float4>()); break;
	default: hipLaunchKernelGGL(k_nearest_gather<3>, query_blocks(nf), dim3(kNearestThreads), 0, st, static_cast<int64_t>(nf), pos, vals2.as<uint32_t>(), t.pts.as<float4>()); break;
	}
	hipLaunchKernelGGL(k_nearest_leaves, query_blocks(P), dim3(kNearestThreads), 0, st, static_cast<int64_t>(nf), P, t.pts.as<float4>(),
	                   t.box.as<float4>());
	for (int64_t first = P / 2; first >= 1; first /= 2) {
		hipLaunchKernelGGL(k_nearest_nodes, query_blocks(first), dim3(kNearestThreads), 0, st, first, t.box.as<float4>());
	}
	FI_HIP_TRY(hipGetLastError());
	FI_HIP_TRY(hipStreamSynchronize(st));  // the temporaries die here
}

const NearestIndex& nearest_of(fi_ctx* c)
{
	if (c->nearest) { return *c->nearest; }
	std::vector<const float*> seg;
	std::vector<int64_t>      cnt;
	int64_t                   n = 0;
	for (const PointBatch* b : c->batches) {
		if (b->n <= 0 || b->prior) { continue; }
		seg.push_back(b->pos.as<float>());
		cnt.push_back(b->n);
		n += b->n;
	}
	NearestIndex* t = new NearestIndex();
	try {
		AllocStream alloc_on(c->stream);
		nearest_build(*t, c->g.ndim, n, seg.data(), cnt.data(), static_cast<int>(seg.size()), c->stream);
	} catch (...) {
		delete t;
		throw;
	}
	c->nearest = t;
	return *t;
}

void nearest_release(fi_ctx* c)
{
	delete c->nearest;
	c->nearest = nullptr;
}

void nearest_query(const NearestIndex& t, int64_t n, const float* queries, float max_distance, float* distances, long long* indices,
                   int memory, hipStream_t st)
{
	if (n == 0) { return; }
	AllocStream alloc_on(st);
	Outputs o(n, distances, indices, memory);
	DevBuf  bq;
	const float* q = queries;
	if (memory == FI_HOST) {
		bq.alloc(sizeof(float) * t.D * n);
		FI_HIP_TRY(hipMemcpyAsync(bq.p, queries, sizeof(float) * t.D * n, hipMemcpyHostToDevice, st));
		q = bq.as<float>();
	}
	QueryArgs a{};
	a.t    = tree_of(t);
	a.n    = n;
	a.q    = q;
	a.lim  = limit_for(max_distance);
	a.dist = o.dist;
	a.idx  = o.idx;
	launch_query<kFromBuffer>(t.D, query_blocks(n), a, st);
	o.finish(st);
}

void nearest_lattice(const NearestIndex& t, const int* sizes, float max_distance, float* distances, long long* indices, int memory,
                     hipStream_t st)
{
	const int D     = t.D;
	int64_t   total = 1, blocks = 1;
	QueryArgs a{};
	for (int d = 0; d < 3; ++d) {
		const int e = D == 1 ? TileShape<1>::e[d] : D == 2 ? TileShape<2>::e[d] : TileShape<3>::e[d];
		a.sz[d]     = d < D ? sizes[d] : 1;
		a.tiles[d]  = (a.sz[d] + e - 1) / e;
		total *= a.sz[d];
		blocks *= a.tiles[d];
	}
	FI_REQUIRE(total < (int64_t(1) << 31), FI_ERR_UNSUPPORTED, "a lattice of %lld points", static_cast<long long>(total));
	AllocStream alloc_on(st);
	Outputs o(total, distances, indices, memory);
	a.t    = tree_of(t);
	a.n    = total;
	a.lim  = limit_for(max_distance);
	a.dist = o.dist;
	a.idx  = o.idx;
	launch_query<kFromLattice>(D, dim3(static_cast<unsigned>(blocks)), a, st);
	o.finish(st);
}

void nearest_lattice_list_d2(const NearestIndex& t, const int* n, int64_t nb, const uint32_t* idx, float* d2, hipStream_t st)
{
	if (nb == 0) { return; }
	QueryArgs a{};
	for (int d = 0; d < 3; ++d) { a.sz[d] = d < t.D ? n[d] : 1; }
	a.t    = tree_of(t);
	a.n    = nb;
	a.list = idx;
	a.lim  = INFINITY;
	a.d2   = d2;
	launch_query<kFromList>(t.D, query_blocks(nb), a, st);
}

}  // namespace fi
