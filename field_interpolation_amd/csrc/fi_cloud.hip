// fi_cloud.hip -- a point cloud made clean on the device: thinning and outlier removal.
//
// The contract (include/fi_hip.h fi_radius_count .. fi_cloud_thin; tests/cloud_reference.py is its definition
// in numpy): s(p, q) is fi_nearest's fp32 sum; a point lies within a radius when s <= limit_for(radius), i.e. when
// sqrtf(s) <= radius; a point's neighbours are the first k pairs (s, j) over the finite points j other than itself; every fp64
// figure is one rounding per operation (-ffp-contract=off) over + - * / sqrt, every sum in a fixed order.  No float atomics:
// a repeated call returns the same bytes.
//
// How it is found:
//   radius     fi_bvh.h's stackless walk over fi_nearest.h's tree, unchanged.  The visitor never lowers the walk's bound, so
//              the cut stays limit_for(radius); it counts the slots it accepts and, once `limit` of them are found, puts the
//              bound below zero: no further node is admitted and the walk unwinds.  No list: the registers of k_nearest_query.
//   neighbours one thread per SORTED SLOT of the tree, as k_knn_normals: a wave's points are Morton neighbours and walk the
//              same nodes; fi_knn_list.h's register-resident list in the classes 8 / 16 / 32.  The point itself is left out by
//              its index, so k neighbours need a list of k, not k + 1.  Results go to the point's own index.
//   statistics fi_treesum.h's fixed-order sum over the means in point order, twice (the mean, then the squared deviations
//              from it); then the mask.  The order of the sums does not know the Morton sort.
//   thinning   no tree: (cell key, index) pairs sorted by key (fi_prim.h's Onesweep, stable: a cell's points ascend), run heads
//              scanned into cell numbers, one thread per cell walking its run; one read-back (error bit and cell count), one
//              device allocation (fi_arena.h) -- fi_simplify.hip's shape.
// The counts of kept points are integer atomics of one add per wave: integers add up the same in any order.
#include "fi_solver_internal.h"
#include "fi_cloud.h"
#include "fi_bvh.h"
#include "fi_knn_list.h"
#include "fi_prim.h"
#include "fi_treesum.h"

#include <algorithm>

namespace fi {

namespace {

using namespace bvh;
using namespace knn;

// ---- points within a radius ---------------------------------------------------------------------------------------------

struct RadiusArgs {
	Tree                t;
	int64_t             n;      // queries (SELF: unused, the tree's nf slots are the queries)
	const float*        q;      // float[n][D]
	float               lim;    // the largest float whose sqrtf is <= radius
	int                 limit;  // counting stops here
	int*                counts; // int[n]
	unsigned char*      keep;   // SELF: uint8[t.n] by point index, or nullptr
	unsigned long long* kept;   // SELF: how many are kept
};

// SELF: thread i takes the point of sorted slot i as its query and leaves that point out by its index; the answer is whether
// `limit` others lie within the radius
template <int D, bool SELF>
__global__ __launch_bounds__(kThreads) void k_cloud_radius(RadiusArgs a)
{
	const int64_t i    = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	bool          kept = false;
	if (i < (SELF ? a.t.nf : a.n)) {
		float    q[D];
		uint32_t me     = kNone;
		bool     finite = true;
		if constexpr (SELF) {
			const float4 self  = a.t.items[i];
			const float  s3[3] = {self.x, self.y, self.z};
			me                 = __float_as_uint(self.w);
#pragma unroll
			for (int d = 0; d < D; ++d) { q[d] = s3[d]; }
		} else {
#pragma unroll
			for (int d = 0; d < D; ++d) { q[d] = a.q[i * D + d]; }
			finite = finite_point<D>(q);
		}
		int c = -1;
		if (finite) {
			c = 0;
			float best;
			search<D, kNearestLeaf>(a.t, q, a.lim, best, [&](int64_t at, float& least) {
				const float4 p  = a.t.items[at];
				const bool   in = c < a.limit && __float_as_uint(p.w) != me && sq_dist<D>(p, q) <= a.lim;
				c += in ? 1 : 0;
				if (c >= a.limit) { least = -1.0f; }  // every lb is >= 0: nothing more is admitted
			});
		}
		if constexpr (SELF) {
			kept = c >= a.limit;
			if (a.keep) { a.keep[me] = kept ? 1 : 0; }
		} else {
			a.counts[i] = c;
		}
	}
	if constexpr (SELF) { treesum::count_flags(kept, a.kept); }
}

template <int D>
void launch_radius(bool self, dim3 grid, const RadiusArgs& a, hipStream_t st)
{
	if (self) {
		hipLaunchKernelGGL((k_cloud_radius<D, true>), grid, dim3(kThreads), 0, st, a);
	} else {
		hipLaunchKernelGGL((k_cloud_radius<D, false>), grid, dim3(kThreads), 0, st, a);
	}
}

void launch_radius(int D, bool self, dim3 grid, const RadiusArgs& a, hipStream_t st)
{
	switch (D) {
	case 1: launch_radius<1>(self, grid, a, st); break;
	case 2: launch_radius<2>(self, grid, a, st); break;
	default: launch_radius<3>(self, grid, a, st); break;
	}
	FI_HIP_TRY(hipGetLastError());
}

// ---- the distances to a point's neighbours ------------------------------------------------------------------------------

struct NeighbourArgs {
	Tree   t;
	int    k;
	float  lim;     // the largest float whose sqrtf is <= max_distance
	float* mean;    // float[t.n] by point index, or nullptr
	float* kth;     // float[t.n], or nullptr
	int*   counts;  // int[t.n], or nullptr
};

template <int D, int CAP>
__global__ __launch_bounds__(kThreads) void k_cloud_neighbours(NeighbourArgs a)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= a.t.nf) { return; }
	const float4   self  = a.t.items[i];
	const float    s3[3] = {self.x, self.y, self.z};
	const uint32_t me    = __float_as_uint(self.w);
	float          q[D];
#pragma unroll
	for (int d = 0; d < D; ++d) { q[d] = s3[d]; }
	List<CAP> b;
	list_reset<CAP>(b, CAP - a.k);
	float bound;
	search<D, kNearestLeaf>(a.t, q, a.lim, bound, [&](int64_t at, float& least) {
		const float4   p = a.t.items[at];
		const uint32_t j = __float_as_uint(p.w);
		if (j != me) { list_offer<CAP>(b, sq_dist<D>(p, q), j, 0u); }
		least = b.s;  // the k-th s: +inf until k pairs are held
	});
	// the distances' sum from 0.0 in result order, divided by their number
	int    m    = 0;
	double sum  = 0.0;
	float  last = INFINITY;
	list_each<CAP>(b, [&](int, float s, uint32_t j, uint32_t) {
		if (!found(s, j, a.lim)) { return; }
		last = sqrtf(s);
		sum  = sum + static_cast<double>(last);
		++m;
	});
	if (a.mean) { a.mean[me] = m > 0 ? static_cast<float>(sum / static_cast<double>(m)) : INFINITY; }
	if (a.kth) { a.kth[me] = last; }
	if (a.counts) { a.counts[me] = m; }
}

// what a point outside the tree (a non-finite one) gets
__global__ __launch_bounds__(kThreads) void k_cloud_blank(int64_t n, float* __restrict__ mean, float* __restrict__ kth, int* __restrict__ counts)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	if (mean) { mean[i] = NAN; }
	if (kth) { kth[i] = NAN; }
	if (counts) { counts[i] = 0; }
}

template <int D>
void launch_neighbours(int cap, dim3 grid, const NeighbourArgs& a, hipStream_t st)
{
	switch (cap) {
	case 8: hipLaunchKernelGGL((k_cloud_neighbours<D, 8>), grid, dim3(kThreads), 0, st, a); break;
	case 16: hipLaunchKernelGGL((k_cloud_neighbours<D, 16>), grid, dim3(kThreads), 0, st, a); break;
	default: hipLaunchKernelGGL((k_cloud_neighbours<D, 32>), grid, dim3(kThreads), 0, st, a); break;
	}
}

// mean / kth / counts (device, t.n each, any of them null) of the set's own points, enqueued on st
void neighbours_on_device(const NearestIndex& t, int k, float max_distance, float* mean, float* kth, int* counts, hipStream_t st)
{
	NeighbourArgs a{};
	a.t      = tree_of(t);
	a.k      = k;
	a.lim    = limit_for(max_distance);
	a.mean   = mean;
	a.kth    = kth;
	a.counts = counts;
	if (t.nf < t.n) { hipLaunchKernelGGL(k_cloud_blank, dim3(blocks_for(t.n)), dim3(kThreads), 0, st, t.n, mean, kth, counts); }
	if (t.nf > 0) {
		const dim3 grid(blocks_for(t.nf));
		switch (t.D) {
		case 1: launch_neighbours<1>(capacity_for(k), grid, a, st); break;
		case 2: launch_neighbours<2>(capacity_for(k), grid, a, st); break;
		default: launch_neighbours<3>(capacity_for(k), grid, a, st); break;
		}
	}
	FI_HIP_TRY(hipGetLastError());
}

// ---- the statistical rule -----------------------------------------------------------------------------------------------

constexpr int kSumBlock = treesum::kChunk;  // the indices a workgroup sums

struct StatState {
	double             mean, stddev, threshold;
	long long          counted;
	unsigned long long kept;
};

// the block sums of the counted x (PASS 0, with their number) or of their squared deviations from the mean (PASS 1); an
// uncounted point and the tail add 0.0.  The number is an integer, no part of the fixed-order sum: it keeps a tree of its own.
template <int PASS>
__global__ __launch_bounds__(kSumBlock) void k_cloud_block_sums(int64_t n, const float* __restrict__ x32, const StatState* __restrict__ state,
                                                                double* __restrict__ part, uint32_t* __restrict__ cnt)
{
	__shared__ double   s[1][kSumBlock];
	__shared__ uint32_t c[kSumBlock];
	const int     t    = threadIdx.x;
	const int64_t i    = static_cast<int64_t>(blockIdx.x) * kSumBlock + t;
	double        v[1] = {0.0};
	uint32_t      m    = 0;
	if (i < n) {
		const double x = static_cast<double>(x32[i]);
		if (isfinite(x)) {
			m = 1;
			if constexpr (PASS == 0) {
				v[0] = x;
			} else {
				const double e = x - state->mean;
				v[0]           = e * e;
			}
		}
	}
	c[t] = m;
	treesum::block_tree<1>(v, s);
	for (int w = kSumBlock / 2; w > 0; w >>= 1) {
		if (t < w) { c[t] += c[t + w]; }
		__syncthreads();
	}
	if (t == 0) {
		part[blockIdx.x] = s[0][0];
		if constexpr (PASS == 0) { cnt[blockIdx.x] = c[0]; }
	}
}

// one wave: the block sums in ascending order, then the mean (PASS 0) or the standard deviation and the threshold (PASS 1)
template <int PASS>
__global__ __launch_bounds__(64) void k_cloud_finish(int64_t nb, const double* __restrict__ part, const uint32_t* __restrict__ cnt, float std_ratio,
                                                     StatState* __restrict__ state)
{
	const int lane = threadIdx.x;
	double    total[1];
	treesum::ordered_sum<1>(part, 1, nb, lane, total);
	long long N = 0;
	if constexpr (PASS == 0) {  // the counts of the blocks lane, lane + 64, ...; then the wave's
		for (int64_t b = lane; b < nb; b += 64) { N += cnt[b]; }
		for (int o = 32; o > 0; o >>= 1) { N += __shfl_xor(N, o, 64); }
	}
	if (lane != 0) { return; }
	if constexpr (PASS == 0) {
		state->counted   = N;
		state->kept      = 0;
		state->mean      = N > 0 ? total[0] / static_cast<double>(N) : 0.0;
		state->stddev    = 0.0;
		state->threshold = 0.0;
	} else {
		N = state->counted;
		if (N > 0) {
			const double sd  = sqrt(total[0] / static_cast<double>(N));
			state->stddev    = sd;
			state->threshold = state->mean + static_cast<double>(std_ratio) * sd;
		}
	}
}

__global__ __launch_bounds__(kThreads) void k_cloud_keep(int64_t n, const float* __restrict__ x32, StatState* state, unsigned char* __restrict__ keep)
{
	const int64_t i    = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	bool          kept = false;
	if (i < n) {
		const double x = static_cast<double>(x32[i]);
		kept           = isfinite(x) && x <= state->threshold;
		if (keep) { keep[i] = kept ? 1 : 0; }
	}
	treesum::count_flags(kept, &state->kept);
}

// ---- thinning -----------------------------------------------------------------------------------------------------------

constexpr int      kCellBias = 1 << 20;  // |cell coordinate| < 2^20: 21 bits an axis (fi_simplify.hip's rule)
constexpr uint32_t kErrRange = 1u;

struct Grid {
	float cell;
	float o[3];
};

// the cell key of every finite point; `sentinel` (above every key) for the others
template <int D>
__global__ __launch_bounds__(kThreads) void k_cloud_thin_keys(int64_t n, const float* __restrict__ pos, Grid g, uint64_t sentinel,
                                                               uint64_t* __restrict__ key, uint32_t* __restrict__ val, uint32_t* info)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	val[i] = static_cast<uint32_t>(i);
	bool     finite = true, inside = true;
	uint64_t k = 0;
#pragma unroll
	for (int d = 0; d < D; ++d) {
		const float p = pos[i * D + d];
		const float c = floorf((p - g.o[d]) / g.cell);
		finite        = finite && isfinite(p);
		const bool in = fabsf(c) < static_cast<float>(kCellBias);  // (false for a NaN)
		inside        = inside && in;
		k |= static_cast<uint64_t>((in ? static_cast<int>(c) : 0) + kCellBias) << (21 * d);
	}
	if (finite && !inside) { atomicOr(info, kErrRange); }
	key[i] = finite && inside ? k : sentinel;
}

__global__ __launch_bounds__(kThreads) void k_cloud_thin_heads(int64_t n, const uint64_t* __restrict__ key, uint64_t sentinel,
                                                                uint32_t* __restrict__ head)
{
	const int64_t s = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (s > n) { return; }
	head[s] = s < n && key[s] != sentinel && (s == 0 || key[s - 1] != key[s]) ? 1u : 0u;  // (entry n: the scan's total)
}

// every point's cell; the start of every cell's run of sorted points (first[nc]: the end of the last); info[1] = nc
__global__ __launch_bounds__(kThreads) void k_cloud_thin_assign(int64_t n, const uint64_t* __restrict__ key, const uint32_t* __restrict__ order,
                                                                 const uint32_t* __restrict__ head, const uint32_t* __restrict__ number,
                                                                 uint64_t sentinel, int* __restrict__ cell_map, uint32_t* __restrict__ first,
                                                                 uint32_t* __restrict__ info)
{
	const int64_t s = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (s > n) { return; }
	if (s < n && key[s] != sentinel) {
		const uint32_t c = number[s] + head[s] - 1u;
		if (cell_map) { cell_map[order[s]] = static_cast<int>(c); }
		if (head[s]) { first[c] = static_cast<uint32_t>(s); }
	} else {
		if (s < n && cell_map) { cell_map[order[s]] = -1; }
		if (s == 0 || key[s - 1] != sentinel) { first[number[s]] = static_cast<uint32_t>(s); }  // (number[s]: every head lies before)
	}
	if (s == n) { info[1] = number[n]; }
}

struct ThinArgs {
	int64_t         nc;
	int             mode;
	const uint32_t* first;   // uint32[nc + 1] into order
	const uint32_t* order;   // the finite points by cell, ascending within one
	const float*    pos;
	const float*    nrm;     // or nullptr
	const float*    val;     // or nullptr
	float*          opos;    // float[nc][D]
	float*          onrm;    // or nullptr
	float*          oval;    // or nullptr
	int*            ocount;  // or nullptr
	long long*      oindex;  // or nullptr
};

template <int D>
__global__ __launch_bounds__(kThreads) void k_cloud_thin_cells(ThinArgs a)
{
	const int64_t c = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (c >= a.nc) { return; }
	const uint32_t b = a.first[c], e = a.first[c + 1];
	const int64_t  lowest = a.order[b];
	if (a.ocount) { a.ocount[c] = static_cast<int>(e - b); }
	if (a.oindex) { a.oindex[c] = lowest; }
	if (a.mode == FI_THIN_FIRST) {
#pragma unroll
		for (int d = 0; d < D; ++d) {
			a.opos[c * D + d] = a.pos[lowest * D + d];
			if (a.onrm) { a.onrm[c * D + d] = a.nrm[lowest * D + d]; }
		}
		if (a.oval) { a.oval[c] = a.val[lowest]; }
		return;
	}
	double sx[D], sn[D], sv = 0.0;
#pragma unroll
	for (int d = 0; d < D; ++d) {
		sx[d] = 0.0;
		sn[d] = 0.0;
	}
	for (uint32_t s = b; s < e; ++s) {
		const int64_t v = a.order[s];
#pragma unroll
		for (int d = 0; d < D; ++d) {
			sx[d] = sx[d] + static_cast<double>(a.pos[v * D + d]);
			if (a.onrm) { sn[d] = sn[d] + static_cast<double>(a.nrm[v * D + d]); }
		}
		if (a.oval) { sv = sv + static_cast<double>(a.val[v]); }
	}
	const double count = static_cast<double>(e - b);
#pragma unroll
	for (int d = 0; d < D; ++d) { a.opos[c * D + d] = static_cast<float>(sx[d] / count); }
	if (a.oval) { a.oval[c] = static_cast<float>(sv / count); }
	if (a.onrm) {
		double l2 = sn[0] * sn[0];
#pragma unroll
		for (int d = 1; d < D; ++d) { l2 = l2 + sn[d] * sn[d]; }
		const double len = sqrt(l2);
#pragma unroll
		for (int d = 0; d < D; ++d) { a.onrm[c * D + d] = len > 0.0 ? static_cast<float>(sn[d] / len) : 0.0f; }
	}
}

using namespace prim;  // Arena, Scratch, scan_u32, sort_u64, bits_for, grid
static_assert(kThreads == kGridThreads, "grid() counts work groups of kThreads");

// the temporaries of a thinning call; with host buffers also the staged inputs and outputs
struct ThinWork {
	uint32_t* info;  // [0]: the error bits, [1]: the number of cells; zeroed
	uint64_t *key, *key2;
	uint32_t *val, *order, *head, *number, *first;
	const float *pos, *nrm, *value;
	float *   opos, *onrm, *ovalue;
	int *     ocount, *map;
	long long* oindex;
	Scratch   tmp;
};

template <int D>
void thin(int64_t n, const float* positions, const float* normals, const float* values, const Grid& g, int mode, float* out_positions,
          float* out_normals, float* out_values, int* out_counts, long long* out_indices, int* cell_map, long* num_out, int memory,
          hipStream_t st)
{
	const uint64_t sentinel  = uint64_t(1) << (21 * D);
	const size_t   tmp_bytes = std::max(sort_bytes(n, 0, 21 * D + 1), scan_bytes(n + 1));
	ThinWork       w{};
	DevBuf         block;
	arena_alloc(block, [&](Arena& a) {
		w.info   = a.take<uint32_t>(2);
		w.key    = a.take<uint64_t>(n);
		w.key2   = a.take<uint64_t>(n);
		w.val    = a.take<uint32_t>(n);
		w.order  = a.take<uint32_t>(n);
		w.head   = a.take<uint32_t>(n + 1);
		w.number = a.take<uint32_t>(n + 1);
		w.first  = a.take<uint32_t>(n + 1);
		w.pos    = stage::in(a, positions, n * D, memory, st);
		w.nrm    = stage::in(a, out_normals ? normals : nullptr, n * D, memory, st);  // (read only for its output)
		w.value  = stage::in(a, out_values ? values : nullptr, n, memory, st);
		w.opos   = stage::out(a, out_positions, n * D, memory);
		w.onrm   = stage::out(a, out_normals, n * D, memory);
		w.ovalue = stage::out(a, out_values, n, memory);
		w.ocount = stage::out(a, out_counts, n, memory);
		w.oindex = stage::out(a, out_indices, n, memory);
		w.map    = stage::out(a, cell_map, n, memory);
		w.tmp.p     = a.take<char>(static_cast<int64_t>(tmp_bytes));
		w.tmp.bytes = tmp_bytes;
	});
	FI_HIP_TRY(hipMemsetAsync(w.info, 0, 2 * sizeof(uint32_t), st));
	hipLaunchKernelGGL(k_cloud_thin_keys<D>, grid(n), dim3(kThreads), 0, st, n, w.pos, g, sentinel, w.key, w.val, w.info);
	FI_HIP_TRY(hipGetLastError());
	sort_u64(w.key, w.key2, w.val, w.order, n, 0, 21 * D + 1, w.tmp, st);
	hipLaunchKernelGGL(k_cloud_thin_heads, grid(n + 1), dim3(kThreads), 0, st, n, w.key2, sentinel, w.head);
	FI_HIP_TRY(hipGetLastError());
	scan_u32(w.head, w.number, n + 1, w.tmp, st);
	hipLaunchKernelGGL(k_cloud_thin_assign, grid(n + 1), dim3(kThreads), 0, st, n, w.key2, w.order, w.head, w.number, sentinel, w.map, w.first,
	                   w.info);
	FI_HIP_TRY(hipGetLastError());
	uint32_t info[2] = {0, 0};
	FI_HIP_TRY(hipMemcpyAsync(info, w.info, sizeof(info), hipMemcpyDeviceToHost, st));
	FI_HIP_TRY(hipStreamSynchronize(st));
	FI_REQUIRE((info[0] & kErrRange) == 0, FI_ERR_INVALID, "a point lies 2^20 cells or more from the origin (cell %g)",
	           static_cast<double>(g.cell));
	const int64_t nc = info[1];
	if (nc > 0) {
		ThinArgs a{};
		a.nc     = nc;
		a.mode   = mode;
		a.first  = w.first;
		a.order  = w.order;
		a.pos    = w.pos;
		a.nrm    = w.nrm;
		a.val    = w.value;
		a.opos   = w.opos;
		a.onrm   = w.onrm;
		a.oval   = w.ovalue;
		a.ocount = w.ocount;
		a.oindex = w.oindex;
		hipLaunchKernelGGL(k_cloud_thin_cells<D>, grid(nc), dim3(kThreads), 0, st, a);
		FI_HIP_TRY(hipGetLastError());
	}
	if (nc > 0) {  // nc rows of the per-cell outputs, n of the map
		stage::back(out_positions, w.opos, D * nc, memory, st);
		stage::back(out_normals, w.onrm, D * nc, memory, st);
		stage::back(out_values, w.ovalue, nc, memory, st);
		stage::back(out_counts, w.ocount, nc, memory, st);
		stage::back(out_indices, w.oindex, nc, memory, st);
	}
	stage::back(cell_map, w.map, n, memory, st);
	FI_HIP_TRY(hipStreamSynchronize(st));
	*num_out = static_cast<long>(nc);
}

}  // namespace

void cloud_radius_count(const NearestIndex& t, int64_t n, const float* queries, float radius, int limit, int* counts, int memory,
                        hipStream_t st)
{
	if (n == 0) { return; }
	AllocStream alloc_on(st);
	stage::Out<int> c(counts, n, memory);
	stage::In<float> q(queries, n * t.D, memory, st);
	RadiusArgs  a{};
	a.t      = tree_of(t);
	a.n      = n;
	a.q      = q;
	a.lim    = limit_for(radius);
	a.limit  = limit;
	a.counts = c.dev;
	launch_radius(t.D, false, dim3(blocks_for(n)), a, st);
	c.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

void cloud_neighbour_distances(const NearestIndex& t, int k, float max_distance, float* mean, float* kth, int* counts, int memory,
                               hipStream_t st)
{
	if (t.n == 0) { return; }
	AllocStream   alloc_on(st);
	stage::Out<float> m(mean, t.n, memory);
	stage::Out<float> kt(kth, t.n, memory);
	stage::Out<int>   c(counts, t.n, memory);
	neighbours_on_device(t, k, max_distance, m.dev, kt.dev, c.dev, st);
	m.back(st);
	kt.back(st);
	c.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

void cloud_outliers_statistical(const NearestIndex& t, int k, float max_distance, float std_ratio, unsigned char* keep,
                                fi_outlier_stats* stats, int memory, hipStream_t st)
{
	if (stats) { *stats = fi_outlier_stats{0, 0, 0.0, 0.0, 0.0}; }
	if (t.n == 0) { return; }
	AllocStream           alloc_on(st);
	stage::Out<unsigned char> kp(keep, t.n, memory);
	const int64_t         nb = (t.n + kSumBlock - 1) / kSumBlock;
	float*                mean  = nullptr;
	double*               part  = nullptr;
	uint32_t*             cnt   = nullptr;
	StatState*            state = nullptr;
	DevBuf                block;
	prim::arena_alloc(block, [&](prim::Arena& a) {
		mean  = a.take<float>(t.n);
		part  = a.take<double>(nb);
		cnt   = a.take<uint32_t>(nb);
		state = a.take<StatState>(1);
	});
	neighbours_on_device(t, k, max_distance, mean, nullptr, nullptr, st);
	const dim3 blocks(static_cast<unsigned>(nb));
	hipLaunchKernelGGL(k_cloud_block_sums<0>, blocks, dim3(kSumBlock), 0, st, t.n, mean, state, part, cnt);
	hipLaunchKernelGGL(k_cloud_finish<0>, dim3(1), dim3(64), 0, st, nb, part, cnt, std_ratio, state);
	hipLaunchKernelGGL(k_cloud_block_sums<1>, blocks, dim3(kSumBlock), 0, st, t.n, mean, state, part, cnt);
	hipLaunchKernelGGL(k_cloud_finish<1>, dim3(1), dim3(64), 0, st, nb, part, cnt, std_ratio, state);
	hipLaunchKernelGGL(k_cloud_keep, dim3(blocks_for(t.n)), dim3(kThreads), 0, st, t.n, mean, state, kp.dev);
	FI_HIP_TRY(hipGetLastError());
	StatState h{};
	FI_HIP_TRY(hipMemcpyAsync(&h, state, sizeof(h), hipMemcpyDeviceToHost, st));
	kp.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
	if (stats) {
		stats->counted   = static_cast<long>(h.counted);
		stats->kept      = static_cast<long>(h.kept);
		stats->mean      = h.mean;
		stats->stddev    = h.stddev;
		stats->threshold = h.threshold;
	}
}

void cloud_outliers_radius(const NearestIndex& t, float radius, int min_neighbours, unsigned char* keep, long* num_kept, int memory,
                           hipStream_t st)
{
	if (num_kept) { *num_kept = 0; }
	if (t.n == 0) { return; }
	AllocStream           alloc_on(st);
	stage::Out<unsigned char> kp(keep, t.n, memory);
	DevBuf                total;
	total.alloc(sizeof(unsigned long long));
	FI_HIP_TRY(hipMemsetAsync(total.p, 0, sizeof(unsigned long long), st));
	if (kp.dev && t.nf < t.n) { FI_HIP_TRY(hipMemsetAsync(kp.dev, 0, t.n, st)); }  // a point outside the tree is not kept
	if (t.nf > 0) {
		RadiusArgs a{};
		a.t     = tree_of(t);
		a.lim   = limit_for(radius);
		a.limit = min_neighbours;
		a.keep  = kp.dev;
		a.kept  = total.as<unsigned long long>();
		launch_radius(t.D, true, dim3(blocks_for(t.nf)), a, st);
	}
	unsigned long long h = 0;
	FI_HIP_TRY(hipMemcpyAsync(&h, total.p, sizeof(h), hipMemcpyDeviceToHost, st));
	kp.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
	if (num_kept) { *num_kept = static_cast<long>(h); }
}

void cloud_thin(int ndim, int64_t n, const float* positions, const float* normals, const float* values, float cell, const float* origin,
                int mode, float* out_positions, float* out_normals, float* out_values, int* out_counts, long long* out_indices,
                int* cell_map, long* num_out, int memory)
{
	*num_out = 0;
	if (n == 0) { return; }
	Grid g{};
	g.cell = cell;
	for (int d = 0; d < ndim; ++d) { g.o[d] = origin ? origin[d] : 0.0f; }
	hipStream_t st = nullptr;
	switch (ndim) {
	case 1:
		thin<1>(n, positions, normals, values, g, mode, out_positions, out_normals, out_values, out_counts, out_indices, cell_map, num_out,
		        memory, st);
		break;
	case 2:
		thin<2>(n, positions, normals, values, g, mode, out_positions, out_normals, out_values, out_counts, out_indices, cell_map, num_out,
		        memory, st);
		break;
	default:
		thin<3>(n, positions, normals, values, g, mode, out_positions, out_normals, out_values, out_counts, out_indices, cell_map, num_out,
		        memory, st);
		break;
	}
}

}  // namespace fi
