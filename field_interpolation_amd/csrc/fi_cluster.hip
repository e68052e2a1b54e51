// fi_cluster.hip -- the clusters of a point cloud on the device: Euclidean clusters and DBSCAN labels, and a table per cluster.
//
// The contract (include/fi_hip.h fi_cluster .. fi_cluster_measure; tests/cluster_reference.py is its
// definition in numpy): s(p, q) is fi_nearest's fp32 sum and a pair lies within eps when s <= limit_for(eps), i.e. when
// sqrtf(s) <= eps; a finite point is core when min_points finite points (itself included) lie within eps of it; clusters are
// the connected components of the core points under that relation, numbered by their lowest core point; a finite point that
// is not core takes the cluster of the first pair (s, j) over the core points j within eps, or -1.  Every output is defined
// bit for bit: nothing here depends on the run or the launch shape.
//
// How it is found:
//   core     fi_bvh.h's stackless walk over fi_nearest.h's tree, one thread per SORTED SLOT (a wave's points are Morton
//            neighbours and walk the same nodes), fi_cloud.hip's radius walk with the point itself counted: the visitor never
//            lowers the bound and, once min_points are found, puts it below zero.  A byte per slot and a byte per point.
//            Not launched for min_points = 1: every finite point is core.
//   join     the same walk from every core slot; a core neighbour with a SMALLER index is united with the point, so a pair
//            is seen from one side only.  fi_unionfind.h's union-find over the point indices: the larger root goes under
//            the smaller by a compare-and-swap, so a cluster's root is its lowest core point whatever the timing.  No LDS,
//            no list.  A second launch jumps every point to its root; root flags are scanned into dense numbers: ascending
//            root index is the contract's numbering.
//   border   a core slot takes its root's number.  Any other slot runs k_nearest_query's shrinking-bound walk limited to eps
//            with a visitor that skips non-core slots and keeps the first (s, j); its label is that point's root's number.
//   measure  no tree: (label, index) pairs sorted by label (fi_prim.h's Onesweep, stable: a cluster's members ascend), every
//            cluster's run found by a binary search, a workgroup per chunk of 256 members summing the coordinates by the
//            fixed tree s[t] += s[t + w], one thread per cluster adding its chunks' partials in ascending order.  One device
//            allocation (fi_arena.h), one read-back (the rows and the error word behind them) -- fi_parts.hip's measuring pass.
// The totals of the stats are integer atomics of one add per wave: integers add up the same in any order.  No float atomics.
#include "fi_solver_internal.h"
#include "fi_cluster.h"
#include "fi_bvh.h"
#include "fi_knn_list.h"
#include "fi_prim.h"
#include "fi_treesum.h"
#include "fi_unionfind.h"

#include <algorithm>
#include <vector>

namespace fi {

namespace {

using namespace bvh;
using namespace unionfind;

// ---- labels ---------------------------------------------------------------------------------------------------------

struct ClusterArgs {
	Tree                 t;
	float                lim;         // the largest float whose sqrtf is <= eps
	int                  min_points;
	unsigned char*       slot_core;   // uint8[t.nf] by sorted slot; nullptr: every finite point is core (min_points = 1)
	unsigned char*       core;        // uint8[n] by point index
	uint32_t*            parent;      // uint32[n] by point index
	const uint32_t*      number;      // uint32[n + 1]: the roots before a point (k_cluster_border)
	int*                 labels;      // int[n] by point index, or nullptr
	unsigned long long*  totals;      // [0]: core points, [1]: border points
};

// the point of sorted slot i as a query
template <int D>
__device__ inline uint32_t slot_point(const Tree& t, int64_t i, float* q)
{
	const float4 self  = t.items[i];
	const float  s3[3] = {self.x, self.y, self.z};
#pragma unroll
	for (int d = 0; d < D; ++d) { q[d] = s3[d]; }
	return __float_as_uint(self.w);
}

__global__ __launch_bounds__(kThreads) void k_cluster_start(int64_t n, uint32_t* __restrict__ parent, unsigned char* __restrict__ core)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	parent[i] = static_cast<uint32_t>(i);
	core[i]   = 0;
}

// whether min_points finite points, the point itself among them, lie within eps of the point of slot i
template <int D>
__global__ __launch_bounds__(kThreads) void k_cluster_core(ClusterArgs a)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= a.t.nf) { return; }
	float          q[D];
	const uint32_t me = slot_point<D>(a.t, i, q);
	int            c  = 0;
	float          best;
	search<D, kNearestLeaf>(a.t, q, a.lim, best, [&](int64_t at, float& least) {
		const bool in = c < a.min_points && sq_dist<D>(a.t.items[at], q) <= a.lim;
		c += in ? 1 : 0;
		if (c >= a.min_points) { least = -1.0f; }  // every lb is >= 0: nothing more is admitted
	});
	const unsigned char is = c >= a.min_points ? 1 : 0;
	a.slot_core[i] = is;
	a.core[me]     = is;
}

// a core point and every core point of a smaller index within eps of it: one set
template <int D>
__global__ __launch_bounds__(kThreads) void k_cluster_join(ClusterArgs a)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= a.t.nf) { return; }
	if (a.slot_core && !a.slot_core[i]) { return; }
	float          q[D];
	const uint32_t me = slot_point<D>(a.t, i, q);
	if (!a.slot_core) { a.core[me] = 1; }
	float best;
	search<D, kNearestLeaf>(a.t, q, a.lim, best, [&](int64_t at, float&) {  // (the bound stays: every slot within eps is seen)
		const float4   p = a.t.items[at];
		const uint32_t j = __float_as_uint(p.w);
		if (j < me && sq_dist<D>(p, q) <= a.lim && (!a.slot_core || a.slot_core[at])) { unite(a.parent, me, j); }
	});
}

// every point straight under its root (roots do not move in this kernel)
__global__ __launch_bounds__(kThreads) void k_cluster_jump(int64_t n, uint32_t* parent)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	for (;;) {
		const uint32_t p = word_load(&parent[i]);
		if (p == i) { break; }
		const uint32_t g = word_load(&parent[p]);
		if (g == p) { break; }
		word_store(&parent[i], g);
	}
}

__global__ __launch_bounds__(kThreads) void k_cluster_roots(int64_t n, const uint32_t* __restrict__ parent, const unsigned char* __restrict__ core,
                                                             uint32_t* __restrict__ flag)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i > n) { return; }
	flag[i] = i < n && core[i] && parent[i] == i ? 1u : 0u;  // (entry n: the scan's total)
}

// the label of the point of slot i: its root's number, or for a point that is not core the number of the root of the first
// (s, j) over the core points within eps
template <int D>
__global__ __launch_bounds__(kThreads) void k_cluster_border(ClusterArgs a)
{
	const int64_t i       = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	bool          is_core = false, is_border = false;
	if (i < a.t.nf) {
		float          q[D];
		const uint32_t me = slot_point<D>(a.t, i, q);
		is_core           = !a.slot_core || a.slot_core[i];
		uint32_t at_core  = me;
		if (!is_core) {
			float best;
			at_core = kNone;
			search<D, kNearestLeaf>(a.t, q, a.lim, best, [&](int64_t at, float& least) {
				if (!a.slot_core[at]) { return; }
				const float4   p = a.t.items[at];
				const float    s = sq_dist<D>(p, q);
				const uint32_t j = __float_as_uint(p.w);
				if (s < least || (s == least && j < at_core)) {
					least   = s;
					at_core = j;
				}
			});
			if (at_core != kNone && best > a.lim) { at_core = kNone; }
			is_border = at_core != kNone;
		}
		if (a.labels) { a.labels[me] = at_core == kNone ? -1 : static_cast<int>(a.number[a.parent[at_core]]); }
	}
	treesum::count_flags(is_core, &a.totals[0]);
	treesum::count_flags(is_border, &a.totals[1]);
}

template <int D>
void launch_labels(const ClusterArgs& a, const dim3 slots, hipStream_t st, int step)
{
	switch (step) {
	case 0: hipLaunchKernelGGL(k_cluster_core<D>, slots, dim3(kThreads), 0, st, a); break;
	case 1: hipLaunchKernelGGL(k_cluster_join<D>, slots, dim3(kThreads), 0, st, a); break;
	default: hipLaunchKernelGGL(k_cluster_border<D>, slots, dim3(kThreads), 0, st, a); break;
	}
}

void launch_labels(int D, const ClusterArgs& a, hipStream_t st, int step)
{
	const dim3 slots(blocks_for(a.t.nf));
	switch (D) {
	case 1: launch_labels<1>(a, slots, st, step); break;
	case 2: launch_labels<2>(a, slots, st, step); break;
	default: launch_labels<3>(a, slots, st, step); break;
	}
	FI_HIP_TRY(hipGetLastError());
}

// ---- the table ------------------------------------------------------------------------------------------------------

constexpr int      kChunk    = treesum::kChunk;  // the contract's chunk of the fixed-order sum: members a workgroup sums, one each
constexpr uint32_t kErrLabel = 1u;

// (label, index) of every point; a point of no cluster gets the key `nc`, behind every cluster's
__global__ __launch_bounds__(kThreads) void k_cluster_keys(int64_t n, int64_t nc, const int* __restrict__ labels, uint64_t* __restrict__ key,
                                                            uint32_t* __restrict__ val, uint32_t* info)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	const int64_t c  = labels[i];
	const bool    in = c >= 0 && c < nc;
	if (!in && c != -1) { atomicOr(info, kErrLabel); }
	key[i] = static_cast<uint64_t>(in ? c : nc);
	val[i] = static_cast<uint32_t>(i);
}

// first[c]: where cluster c begins in the sorted list, c = 0 .. nc (first[nc]: where the last one ends); nchunks[c]: its
// chunks (entry nc: 0, the scan's total)
__global__ __launch_bounds__(kThreads) void k_cluster_first(int64_t n, int64_t nc, const uint64_t* __restrict__ key, uint32_t* __restrict__ first)
{
	const int64_t c = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (c > nc) { return; }
	int64_t lo = 0, hi = n;  // the first entry whose key is >= c
	while (lo < hi) {
		const int64_t mid = (lo + hi) / 2;
		if (key[mid] < static_cast<uint64_t>(c)) {
			lo = mid + 1;
		} else {
			hi = mid;
		}
	}
	first[c] = static_cast<uint32_t>(lo);
}

__global__ __launch_bounds__(kThreads) void k_cluster_chunk_counts(int64_t nc, const uint32_t* __restrict__ first, uint32_t* __restrict__ nchunks)
{
	const int64_t c = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (c > nc) { return; }
	nchunks[c] = treesum::chunks_of(first, c, nc);
}

struct ChunkPartial {
	double   sum[3];
	float    lo[3], hi[3];
	uint32_t core;
};

// one workgroup per chunk: chunk j of cluster c holds the cluster's sorted members [kChunk j, kChunk (j + 1)), one a thread.
// The coordinates are summed by the tree s[t] += s[t + w], w = 128 .. 1, a missing member adding 0.0.
template <int D>
__global__ __launch_bounds__(kChunk) void k_cluster_chunks(int64_t nc, const uint32_t* __restrict__ first, const uint32_t* __restrict__ chunk_first,
                                                            const uint32_t* __restrict__ order, const float* __restrict__ pos,
                                                            const unsigned char* __restrict__ core, ChunkPartial* __restrict__ out)
{
	__shared__ double   s_sum[D][kChunk];
	__shared__ float    s_lo[D][kChunk], s_hi[D][kChunk];
	__shared__ uint32_t s_core[kChunk];
	const uint32_t chunk = blockIdx.x;
	if (chunk >= chunk_first[nc]) { return; }  // (the grid is the bound n / kChunk + nc: the whole workgroup leaves)
	const int64_t  lo    = treesum::owner_of(chunk_first, nc, chunk);  // the cluster of this chunk
	const uint32_t begin = first[lo] + (chunk - chunk_first[lo]) * kChunk, end = first[lo + 1];
	const int      t     = threadIdx.x;
	const uint32_t s     = begin + t;
	double         x[D];
	float          bl[D], bh[D];
	uint32_t       is = 0;
#pragma unroll
	for (int d = 0; d < D; ++d) {
		x[d]  = 0.0;
		bl[d] = INFINITY;
		bh[d] = -INFINITY;
	}
	if (s < end) {
		const int64_t v = order[s];
#pragma unroll
		for (int d = 0; d < D; ++d) {
			const float f = pos[v * D + d];
			x[d]          = static_cast<double>(f);
			bl[d]         = f;
			bh[d]         = f;
		}
		is = core && core[v] ? 1u : 0u;
	}
#pragma unroll
	for (int d = 0; d < D; ++d) {
		s_sum[d][t] = x[d];
		s_lo[d][t]  = bl[d];
		s_hi[d][t]  = bh[d];
	}
	s_core[t] = is;
	__syncthreads();
	for (int w = kChunk / 2; w > 0; w >>= 1) {
		if (t < w) {
#pragma unroll
			for (int d = 0; d < D; ++d) {
				s_sum[d][t] = s_sum[d][t] + s_sum[d][t + w];
				s_lo[d][t]  = fminf(s_lo[d][t], s_lo[d][t + w]);
				s_hi[d][t]  = fmaxf(s_hi[d][t], s_hi[d][t + w]);
			}
			s_core[t] += s_core[t + w];
		}
		__syncthreads();
	}
	if (t == 0) {
		ChunkPartial r{};
#pragma unroll
		for (int d = 0; d < D; ++d) {
			r.sum[d] = s_sum[d][0];
			r.lo[d]  = s_lo[d][0];
			r.hi[d]  = s_hi[d][0];
		}
		r.core     = s_core[0];
		out[chunk] = r;
	}
}

// one thread per cluster: its chunks in ascending order, and its row; the thread behind the last cluster leaves the error
// word in a row of its own
__global__ __launch_bounds__(kThreads) void k_cluster_rows(int64_t nc, const uint32_t* __restrict__ first, const uint32_t* __restrict__ chunk_first,
                                                            const ChunkPartial* __restrict__ partial, const uint32_t* __restrict__ info,
                                                            fi_cluster_row* __restrict__ rows)
{
	const int64_t c = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (c > nc) { return; }
	fi_cluster_row o{};
	if (c == nc) {
		o.count = static_cast<long>(info[0]);
		rows[c] = o;
		return;
	}
	const uint32_t b = chunk_first[c], e = chunk_first[c + 1];
	if (b < e) {
		double    sum[3] = {0.0, 0.0, 0.0};
		long long cores  = 0;
		for (int d = 0; d < 3; ++d) {
			o.lo[d] = INFINITY;
			o.hi[d] = -INFINITY;
		}
		for (uint32_t k = b; k < e; ++k) {
			const ChunkPartial q = partial[k];
			for (int d = 0; d < 3; ++d) {
				sum[d]  = sum[d] + q.sum[d];
				o.lo[d] = fminf(o.lo[d], q.lo[d]);
				o.hi[d] = fmaxf(o.hi[d], q.hi[d]);
			}
			cores += q.core;
		}
		const long long count = static_cast<long long>(first[c + 1]) - static_cast<long long>(first[c]);
		o.count = static_cast<long>(count);
		o.core  = static_cast<long>(cores);
		for (int d = 0; d < 3; ++d) { o.centroid[d] = sum[d] / static_cast<double>(count); }
	}
	rows[c] = o;
}

using namespace prim;  // Arena, Scratch, scan_u32, sort_u64, bits_for, grid
static_assert(kThreads == kGridThreads, "grid() counts work groups of kThreads");

struct MeasureWork {
	uint32_t*       info;  // the error bits; zeroed
	uint64_t *      key, *key2;
	uint32_t *      val, *order, *first, *nchunks, *chunk_first;
	const float*    pos;
	const int*      labels;
	const unsigned char* core;
	ChunkPartial*   partial;
	fi_cluster_row* rows;
	Scratch         tmp;
};

template <int D>
void measure(int64_t n, const float* positions, const int* labels, const unsigned char* core, int64_t nc, fi_cluster_row* rows, int memory,
             hipStream_t st)
{
	const int     bits   = bits_for(nc + 1);
	const int64_t chunks = n / kChunk + nc + 1;  // at most n / kChunk full chunks and a partial one per cluster
	MeasureWork   w{};
	w.tmp.bytes = std::max(sort_bytes(n, 0, bits), scan_bytes(nc + 1));
	DevBuf block;
	arena_alloc(block, [&](Arena& a) {
		w.info        = a.take<uint32_t>(1);
		w.key         = a.take<uint64_t>(n);
		w.key2        = a.take<uint64_t>(n);
		w.val         = a.take<uint32_t>(n);
		w.order       = a.take<uint32_t>(n);
		w.first       = a.take<uint32_t>(nc + 1);
		w.nchunks     = a.take<uint32_t>(nc + 1);
		w.chunk_first = a.take<uint32_t>(nc + 1);
		w.pos         = stage::in(a, positions, n * D, memory, st);
		w.labels      = stage::in(a, labels, n, memory, st);
		w.core        = stage::in(a, core, n, memory, st);
		w.partial     = a.take<ChunkPartial>(chunks);
		w.rows        = a.take<fi_cluster_row>(nc + 1);
		w.tmp.p       = a.take<char>(static_cast<int64_t>(w.tmp.bytes));
	});
	FI_HIP_TRY(hipMemsetAsync(w.info, 0, sizeof(uint32_t), st));
	hipLaunchKernelGGL(k_cluster_keys, grid(n), dim3(kThreads), 0, st, n, nc, w.labels, w.key, w.val, w.info);
	FI_HIP_TRY(hipGetLastError());
	sort_u64(w.key, w.key2, w.val, w.order, n, 0, bits, w.tmp, st);
	hipLaunchKernelGGL(k_cluster_first, grid(nc + 1), dim3(kThreads), 0, st, n, nc, w.key2, w.first);
	hipLaunchKernelGGL(k_cluster_chunk_counts, grid(nc + 1), dim3(kThreads), 0, st, nc, w.first, w.nchunks);
	FI_HIP_TRY(hipGetLastError());
	scan_u32(w.nchunks, w.chunk_first, nc + 1, w.tmp, st);
	if (nc > 0) {
		hipLaunchKernelGGL(k_cluster_chunks<D>, dim3(static_cast<unsigned>(chunks)), dim3(kChunk), 0, st, nc, w.first, w.chunk_first, w.order,
		                   w.pos, w.core, w.partial);
	}
	hipLaunchKernelGGL(k_cluster_rows, grid(nc + 1), dim3(kThreads), 0, st, nc, w.first, w.chunk_first, w.partial, w.info, w.rows);
	FI_HIP_TRY(hipGetLastError());
	std::vector<fi_cluster_row> got(static_cast<size_t>(nc + 1));
	FI_HIP_TRY(hipMemcpyAsync(got.data(), w.rows, sizeof(fi_cluster_row) * (nc + 1), hipMemcpyDeviceToHost, st));
	FI_HIP_TRY(hipStreamSynchronize(st));
	FI_REQUIRE((got[static_cast<size_t>(nc)].count & kErrLabel) == 0, FI_ERR_INVALID, "a label lies outside [-1, %lld)",
	           static_cast<long long>(nc));
	std::copy(got.begin(), got.end() - 1, rows);
}

}  // namespace

void cluster_labels(const NearestIndex& t, float eps, int min_points, int* labels, unsigned char* core, fi_cluster_stats* stats,
                    int memory, hipStream_t st)
{
	if (stats) { *stats = fi_cluster_stats{0, 0, 0, 0, static_cast<long>(t.n - t.nf)}; }
	if (t.n == 0) { return; }
	const int64_t             n = t.n;
	AllocStream               alloc_on(st);
	stage::Out<int>           lb(labels, n, memory);
	stage::Out<unsigned char> cr(core, n, memory);
	ClusterArgs               a{};
	uint32_t*                 flag   = nullptr;
	uint32_t*                 number = nullptr;
	prim::Scratch             tmp;
	tmp.bytes = prim::scan_bytes(n + 1);
	DevBuf block;
	prim::arena_alloc(block, [&](prim::Arena& ar) {
		a.totals    = ar.take<unsigned long long>(2);
		a.parent    = ar.take<uint32_t>(n);
		a.core      = cr.dev ? cr.dev : ar.take<unsigned char>(n);
		a.slot_core = min_points > 1 ? ar.take<unsigned char>(t.nf) : nullptr;
		flag        = ar.take<uint32_t>(n + 1);
		number      = ar.take<uint32_t>(n + 1);
		tmp.p       = ar.take<char>(static_cast<int64_t>(tmp.bytes));
	});
	a.t          = tree_of(t);
	a.lim        = limit_for(eps);
	a.min_points = min_points;
	a.number     = number;
	a.labels     = lb.dev;
	FI_HIP_TRY(hipMemsetAsync(a.totals, 0, 2 * sizeof(unsigned long long), st));
	if (lb.dev && t.nf < n) { FI_HIP_TRY(hipMemsetAsync(lb.dev, 0xFF, sizeof(int) * n, st)); }  // a point outside the tree: -1
	hipLaunchKernelGGL(k_cluster_start, dim3(blocks_for(n)), dim3(kThreads), 0, st, n, a.parent, a.core);
	FI_HIP_TRY(hipGetLastError());
	if (t.nf > 0) {
		if (a.slot_core) { launch_labels(t.D, a, st, 0); }
		launch_labels(t.D, a, st, 1);
	}
	hipLaunchKernelGGL(k_cluster_jump, dim3(blocks_for(n)), dim3(kThreads), 0, st, n, a.parent);
	hipLaunchKernelGGL(k_cluster_roots, dim3(blocks_for(n + 1)), dim3(kThreads), 0, st, n, a.parent, a.core, flag);
	FI_HIP_TRY(hipGetLastError());
	prim::scan_u32(flag, number, n + 1, tmp, st);
	if (t.nf > 0) { launch_labels(t.D, a, st, 2); }
	unsigned long long totals[2] = {0, 0};
	uint32_t           clusters  = 0;
	FI_HIP_TRY(hipMemcpyAsync(totals, a.totals, sizeof(totals), hipMemcpyDeviceToHost, st));
	FI_HIP_TRY(hipMemcpyAsync(&clusters, number + n, sizeof(clusters), hipMemcpyDeviceToHost, st));
	lb.back(st);
	cr.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
	if (stats) {
		stats->clusters = static_cast<long>(clusters);
		stats->core     = static_cast<long>(totals[0]);
		stats->border   = static_cast<long>(totals[1]);
		stats->noise    = static_cast<long>(t.nf) - stats->core - stats->border;
	}
}

void cluster_measure(int ndim, int64_t n, const float* positions, const int* labels, const unsigned char* core, int64_t num_clusters,
                     fi_cluster_row* rows, int memory)
{
	for (int64_t c = 0; c < num_clusters; ++c) { rows[c] = fi_cluster_row{}; }
	if (n == 0) { return; }
	hipStream_t st = nullptr;
	switch (ndim) {
	case 1: measure<1>(n, positions, labels, core, num_clusters, rows, memory, st); break;
	case 2: measure<2>(n, positions, labels, core, num_clusters, rows, memory, st); break;
	default: measure<3>(n, positions, labels, core, num_clusters, rows, memory, st); break;
	}
}

}  // namespace fi
