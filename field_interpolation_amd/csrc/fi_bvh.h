// fi_bvh.h -- the search core of the exact nearest-item queries: fi_nearest.hip (points) and fi_surface.hip (segments and
// triangles) build and walk the same tree; each supplies its items (below) and its per-item distance.
//
// Structure: the usable items sorted by a Morton code over their own bounding box (rocPRIM radix sort), stored in sorted
// order, leaves of kLeaf consecutive items and an implicit balanced binary tree over them (heap numbering: root 1, children
// 2k and 2k + 1, 2^H leaves, empty ones at the end).  Node k keeps its box as two float4 (lo, hi) at box[2k], box[2k + 1];
// the boxes come from a level-by-level min / max reduction: no atomics, the same tree on every run.
//
// Query: one thread per query, depth first, the near child first, a node pruned only when its lower bound lb > best (strict:
// an equal s in another leaf may still carry a smaller index).  s is the fp32 sum from 0.0f of the squared per-axis
// differences to an item's closest point in ascending axes, one rounding per operation (-ffp-contract=off); lb is formed
// like s from the per-axis gaps lo - q / q - hi.  The closest point lies inside its item's box, hence inside every enclosing
// node box; rounding is monotone, so lb <= s holds bit for bit for every item of the box and no margin is needed.  The walk
// keeps no stack: going up is k >> 1 and the sibling is k ^ 1, and one bit per level says whether the sibling has been
// looked at yet -- two registers instead of a stack indexed at run time (which would spill).
//
// Everything here is a template or has internal linkage: both units include it.
#pragma once

#include "fi_solver_internal.h"
#include "fi_prim.h"
#include "fi_stage.h"

#include <cmath>

namespace fi {
namespace bvh {

constexpr int      kBoundsBlocks = 256;
constexpr uint32_t kNone         = 0xFFFFFFFFu;

// Morton bits per axis and the key of an unusable item (sorted behind every usable one)
__host__ __device__ constexpr int morton_bits(int D) { return D == 3 ? 21 : 24; }
__host__ __device__ constexpr uint64_t unusable_key(int D) { return uint64_t(1) << (D * morton_bits(D)); }

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

// ---- the build --------------------------------------------------------------------------------------------------------
//
// An item set `Items` is passed to the kernels by value and supplies
//   kDim, kLeaf      the dimension; items per leaf
//   kVerts           vertices (kDim floats each) of an item as load() returns them: all of them extend the bounds
//   kSlots, kIds     float4 per stored item; whether the items' indices go to an array of their own
//   kBoxAxes         the axes a leaf box spans (the others stay 0)
//   int load(i, v)            item i's vertices into v; 0: usable, 1: unusable (left out of the tree), 2: unusable and counted as bad
//   void key_point(v, m)      the point whose Morton code sorts the item, as doubles
//   void store(i, j, v, items, ids)   item j (its vertices v) as sorted slot i
//   static void extend(items, i, lo, hi)   slot i's contribution to its leaf's box
//   void check(counts, n)     host: the counts {usable, bad} of n items, read back

// bounds of the usable items: per-block partials (lo[3], hi[3]; usable count, bad count) ...
template <class Items>
__global__ __launch_bounds__(kThreads) void k_bvh_bounds(Items it, int64_t n, float* __restrict__ part, uint32_t* __restrict__ cnt)
{
	constexpr int D = Items::kDim;
	__shared__ float    s_lo[3][kThreads], s_hi[3][kThreads];
	__shared__ uint32_t s_n[2][kThreads];
	float    lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
	uint32_t m = 0, bad = 0;
	for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kThreads) {
		float     v[Items::kVerts * D];
		const int r = it.load(i, v);
		bad += r == 2 ? 1u : 0u;
		if (r != 0) { continue; }
		++m;
#pragma unroll
		for (int k = 0; k < Items::kVerts; ++k) {
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
	for (int w = kThreads / 2; w > 0; w >>= 1) {
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

namespace {

// ... and their reduction by one block: bounds part[6 kBoundsBlocks ..), the counts cnt[2 kBoundsBlocks], cnt[2 kBoundsBlocks + 1]
__global__ __launch_bounds__(kBoundsBlocks) void k_bvh_bounds_total(float* __restrict__ part, uint32_t* __restrict__ cnt)
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

// the boxes of the nodes [first, 2 first) of one level from their children
__global__ __launch_bounds__(kThreads) void k_bvh_nodes(int64_t first, float4* __restrict__ box)
{
	const int64_t k = first + static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (k >= 2 * first) { return; }
	const float4 l0 = box[4 * k], h0 = box[4 * k + 1], l1 = box[4 * k + 2], h1 = box[4 * k + 3];
	box[2 * k]     = make_float4(fminf(l0.x, l1.x), fminf(l0.y, l1.y), fminf(l0.z, l1.z), 0.0f);
	box[2 * k + 1] = make_float4(fmaxf(h0.x, h1.x), fmaxf(h0.y, h1.y), fmaxf(h0.z, h1.z), 0.0f);
}

}  // namespace

template <class Items>
__global__ __launch_bounds__(kThreads) void k_bvh_morton(Items it, int64_t n, const float* __restrict__ bounds, uint64_t* __restrict__ keys,
                                                          uint32_t* __restrict__ vals)
{
	constexpr int D = Items::kDim;
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	float    v[Items::kVerts * D];
	uint64_t key = unusable_key(D);
	if (it.load(i, v) == 0) {
		constexpr double top = static_cast<double>((1u << morton_bits(D)) - 1u);
		double           m[D];
		it.key_point(v, m);
		key = 0;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			const double lo = bounds[d], ext = static_cast<double>(bounds[3 + d]) - lo;
			const double u  = ext > 0.0 ? (m[d] - lo) * (top / ext) : 0.0;
			const uint32_t b = static_cast<uint32_t>(fmin(fmax(u, 0.0), top));
			key |= spread(b, D) << d;
		}
	}
	keys[i] = key;
	vals[i] = static_cast<uint32_t>(i);
}

// the usable items in sorted order
template <class Items>
__global__ __launch_bounds__(kThreads) void k_bvh_gather(Items it, int64_t nf, const uint32_t* __restrict__ order, float4* __restrict__ items,
                                                          uint32_t* __restrict__ ids)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= nf) { return; }
	const uint32_t j = order[i];
	float          v[Items::kVerts * Items::kDim];
	(void)it.load(j, v);  // (usable: sorted before every unusable one)
	it.store(i, j, v, items, ids);
}

// the boxes of the leaves (node P + j; an empty leaf gets lo = +inf > hi = -inf)
template <class Items>
__global__ __launch_bounds__(kThreads) void k_bvh_leaves(int64_t nf, int64_t P, const float4* __restrict__ items, float4* __restrict__ box)
{
	const int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (j >= P) { return; }
	constexpr bool flat = Items::kBoxAxes < 3;
	float4 lo = make_float4(INFINITY, INFINITY, flat ? 0.0f : INFINITY, 0.0f), hi = make_float4(-INFINITY, -INFINITY, flat ? 0.0f : -INFINITY, 0.0f);
	const int64_t b = j * Items::kLeaf, e = b + Items::kLeaf < nf ? b + Items::kLeaf : nf;
	for (int64_t i = b; i < e; ++i) { Items::extend(items, i, lo, hi); }
	box[2 * (P + j)]     = lo;
	box[2 * (P + j) + 1] = hi;
}

// The build: bounds, Morton keys, the sort, the usable count read back, the gather into `t.items` (and `t.ids`), the leaf
// boxes and the node levels.  t.nf == 0 afterwards: no usable item, no tree.
template <class Items>
void build(BvhIndex& t, const Items& it, int64_t n, hipStream_t st)
{
	constexpr int D = Items::kDim;
	DevBuf part, cnt, keys, keys2, vals, vals2, tmp;
	part.alloc(sizeof(float) * 6 * (kBoundsBlocks + 1));
	cnt.alloc(sizeof(uint32_t) * 2 * (kBoundsBlocks + 1));
	hipLaunchKernelGGL(k_bvh_bounds<Items>, dim3(kBoundsBlocks), dim3(kThreads), 0, st, it, n, part.as<float>(), cnt.as<uint32_t>());
	hipLaunchKernelGGL(k_bvh_bounds_total, dim3(1), dim3(kBoundsBlocks), 0, st, part.as<float>(), cnt.as<uint32_t>());
	keys.alloc(sizeof(uint64_t) * n);
	keys2.alloc(sizeof(uint64_t) * n);
	vals.alloc(sizeof(uint32_t) * n);
	vals2.alloc(sizeof(uint32_t) * n);
	hipLaunchKernelGGL(k_bvh_morton<Items>, dim3(blocks_for(n)), dim3(kThreads), 0, st, it, n, part.as<float>() + 6 * kBoundsBlocks,
	                   keys.as<uint64_t>(), vals.as<uint32_t>());
	FI_HIP_TRY(hipGetLastError());
	const int end_bit = D * morton_bits(D) + 1;
	tmp.alloc(prim::sort_bytes(n, 0, end_bit));
	prim::sort_u64(keys.as<uint64_t>(), keys2.as<uint64_t>(), vals.as<uint32_t>(), vals2.as<uint32_t>(), n, 0, end_bit,
	               prim::Scratch{tmp.p, tmp.bytes}, st);
	uint32_t c[2] = {0, 0};
	FI_HIP_TRY(hipMemcpyAsync(c, cnt.as<uint32_t>() + 2 * kBoundsBlocks, sizeof(c), hipMemcpyDeviceToHost, st));
	FI_HIP_TRY(hipStreamSynchronize(st));
	it.check(c, n);
	t.nf = c[0];
	if (t.nf == 0) { return; }
	const int64_t leaves = (t.nf + Items::kLeaf - 1) / Items::kLeaf;
	while ((int64_t(1) << t.H) < leaves) { ++t.H; }
	const int64_t P = int64_t(1) << t.H;
	t.items.alloc(sizeof(float4) * Items::kSlots * t.nf);
	if (Items::kIds) { t.ids.alloc(sizeof(uint32_t) * t.nf); }
	t.box.alloc(sizeof(float4) * 4 * P);
	hipLaunchKernelGGL(k_bvh_gather<Items>, dim3(blocks_for(t.nf)), dim3(kThreads), 0, st, it, t.nf, vals2.as<uint32_t>(),
	                   t.items.as<float4>(), t.ids.as<uint32_t>());
	hipLaunchKernelGGL(k_bvh_leaves<Items>, dim3(blocks_for(P)), dim3(kThreads), 0, st, t.nf, P, t.items.as<float4>(), t.box.as<float4>());
	for (int64_t first = P / 2; first >= 1; first /= 2) {
		hipLaunchKernelGGL(k_bvh_nodes, dim3(blocks_for(first)), dim3(kThreads), 0, st, first, t.box.as<float4>());
	}
	FI_HIP_TRY(hipGetLastError());
	FI_HIP_TRY(hipStreamSynchronize(st));  // the temporaries die here
}

// ---- the walk ---------------------------------------------------------------------------------------------------------

// what a query kernel reads of a BvhIndex
struct Tree {
	const float4*   items;
	const uint32_t* ids;
	const float4*   box;
	int64_t         nf;
	uint32_t        P;
	int             H;
};

inline Tree tree_of(const BvhIndex& t)
{
	return Tree{t.items.as<float4>(), t.ids.as<uint32_t>(), t.box.as<float4>(), t.nf, static_cast<uint32_t>(uint32_t(1) << t.H), t.H};
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

// the search of one finite query: visit(i, best) judges sorted slot i and lowers best (the minimum of s so far, +inf at the
// start) along with whatever else the unit tracks; lim: prune nodes with lb > lim as well (sqrtf(lb) > max_distance)
template <int D, int LEAF, class Visit>
__device__ inline void search(const Tree& t, const float* q, float lim, float& best, Visit&& visit)
{
	best = INFINITY;
	if (t.nf == 0) { return; }
	float lb;
	if (!node_lb<D>(t, 1, q, &lb) || lb > lim) { return; }
	uint32_t k = 1, second = 0;
	int      depth = 0;
	for (;;) {
		// node k is admitted: visit it
		if (depth == t.H) {
			const int64_t b = static_cast<int64_t>(k - t.P) * LEAF;
			const int64_t e = b + LEAF < t.nf ? b + LEAF : t.nf;
			for (int64_t i = b; i < e; ++i) { visit(i, best); }
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

// ---- the queries ------------------------------------------------------------------------------------------------------

// sqrtf(lb) > max_distance  <=>  lb > lim: the largest float whose (correctly rounded) square root is <= max_distance
inline float limit_for(float max_distance)
{
	if (std::isinf(max_distance)) { return INFINITY; }
	const double sq = static_cast<double>(max_distance) * max_distance;
	float        x  = sq > 3.4e38 ? INFINITY : static_cast<float>(sq);
	while (x > 0.0f && std::sqrt(x) > max_distance) { x = std::nextafter(x, 0.0f); }
	while (std::sqrt(std::nextafter(x, INFINITY)) <= max_distance) { x = std::nextafter(x, INFINITY); }
	return x;
}

// the tile of kThreads lattice points a block walks (x fastest): coherent queries in a workgroup
template <int D>
struct TileShape;
template <>
struct TileShape<1> { static constexpr int e[3] = {256, 1, 1}; };
template <>
struct TileShape<2> { static constexpr int e[3] = {16, 16, 1}; };
template <>
struct TileShape<3> { static constexpr int e[3] = {8, 8, 4}; };

struct Lattice {
	int     sz[3];
	int64_t tiles[3];  // tiles per axis
};

// the lattice's tiles and its points; the grid of blocks
inline dim3 lattice_grid(int D, const int* sizes, Lattice& l, int64_t* total)
{
	int64_t blocks = 1;
	*total = 1;
	for (int d = 0; d < 3; ++d) {
		const int e = D == 1 ? TileShape<1>::e[d] : D == 2 ? TileShape<2>::e[d] : TileShape<3>::e[d];
		l.sz[d]     = d < D ? sizes[d] : 1;
		l.tiles[d]  = (l.sz[d] + e - 1) / e;
		*total *= l.sz[d];
		blocks *= l.tiles[d];
	}
	FI_REQUIRE(*total < (int64_t(1) << 31), FI_ERR_UNSUPPORTED, "a lattice of %lld points", static_cast<long long>(*total));
	return dim3(static_cast<unsigned>(blocks));
}

// this thread's lattice point as its query q and its linear index; false outside the lattice
template <int D>
__device__ inline bool lattice_query(const Lattice& l, float* q, int64_t* out)
{
	int64_t b = blockIdx.x;
	int     c[3];
	int     tid = threadIdx.x;
	bool    in  = true;
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		const int64_t tc = b % l.tiles[d];
		b /= l.tiles[d];
		c[d] = static_cast<int>(tc) * TileShape<D>::e[d] + tid % TileShape<D>::e[d];
		tid /= TileShape<D>::e[d];
		in   = in && c[d] < l.sz[d];
	}
	if (!in) { return false; }
	*out = c[0] + static_cast<int64_t>(l.sz[0]) * (c[1] + static_cast<int64_t>(l.sz[1]) * c[2]);
#pragma unroll
	for (int d = 0; d < D; ++d) { q[d] = static_cast<float>(c[d]); }
	return true;
}

template <int D>
__device__ inline bool finite_point(const float* p)
{
	bool ok = true;
#pragma unroll
	for (int d = 0; d < D; ++d) { ok = ok && isfinite(p[d]); }
	return ok;
}

// the distance a query writes: best = NaN for a non-finite query, else the search's, with its index bidx -- dropped
// (kNone, +inf) when it lies beyond max_distance
__device__ inline float distance_of(bool finite, float best, float lim, uint32_t& bidx)
{
	if (!finite) { return best; }
	if (bidx != kNone && best > lim) { bidx = kNone; }
	// (a finite item whose s overflows is still the nearest: +inf with its index)
	return bidx == kNone ? INFINITY : sqrtf(best);
}

__device__ inline long long index_of(uint32_t bidx) { return bidx == kNone ? -1LL : static_cast<long long>(bidx); }

// the three outputs of a query on the device (fi_stage.h): the caller's or staged, copied back by finish(), which also ends
// the call; indices and closest (n x D) may be null
struct Outputs {
	stage::Out<float>     dist;
	stage::Out<long long> idx;
	stage::Out<float>     cl;
	Outputs(int64_t n, int D, float* distances, long long* indices, float* closest, int memory)
	    : dist(distances, n, memory), idx(indices, n, memory), cl(closest, D * n, memory)
	{
	}
	void finish(hipStream_t st)
	{
		dist.back(st);
		idx.back(st);
		cl.back(st);
		FI_HIP_TRY(hipStreamSynchronize(st));
	}
};

}  // namespace bvh
}  // namespace fi
