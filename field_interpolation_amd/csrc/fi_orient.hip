// fi_orient.hip -- one consistent sign for the normals of a point cloud, on the device, without a guide.
//
// The contract (include/fi_hip.h fi_orient_normals; tests/orient_reference.py is its definition in numpy):
// the live points' k-nearest-neighbour graph, every edge valued by the agreement a = |n_i . n_j| of the two normal LINES
// (fp64 from the fp32 normals, one rounding per operation: -ffp-contract=off), the minimum spanning forest under the strict
// order (a descending, lo ascending, hi ascending), signs t_i along the forest's edges (a forest edge with n_i . n_j < 0
// flips), and one sign per component from the extreme rule or the guides' vote.  The order is strict, so the forest is
// unique and the result does not depend on how it is found.
//
// How it is found: Boruvka rounds.  Every vertex keeps ONE 32-bit word (representative << 1 | parity relative to it), read
// and written whole, so that concurrent pointer jumping always sees a consistent pair.  A round is four launches:
//   propose   every usable slot (i, r) of the neighbour table whose ends lie in different components offers (~bits(a), lo) to BOTH
//             ends' components by a 64-bit atomicMin (an edge listed from one side only is still seen by the other side);
//             a slot whose ends have met is retired;
//   select    the slots that match their component's minimum offer hi by a 32-bit atomicMin: the component's edge
//             (a, lo, hi) is now the minimum of the 96-bit order;
//   hook      every root hangs itself onto the other end's component with parity par(u) ^ flip ^ par(v) -- except that of two
//             components that picked each other (then it is the same edge) the smaller representative stays root.  Reads
//             the old words, writes a second array: no root is read while it is rewritten;
//   jump      every vertex halves its path (XOR-ing the parities) until its parent is a root, and resets its offers.
// The host reads one counter a round and stops after the first round that hooked nothing.
#include "fi_solver_internal.h"
#include "fi_orient.h"
#include "fi_bvh.h"

#include <cstdio>

namespace fi {

namespace {

using namespace bvh;

constexpr uint64_t kNoOffer = ~uint64_t(0);

__device__ inline uint32_t word_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void word_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// (values only ever fall: a plain read that is not below `v` already can only be stale on the high side)
__device__ inline void lower64(unsigned long long* p, unsigned long long v)
{
	if (*p > v) { atomicMin(p, v); }
}
__device__ inline void lower32(uint32_t* p, uint32_t v)
{
	if (*p > v) { atomicMin(p, v); }
}

// d of the contract for the normals of points i and j
template <int D>
__device__ inline double line_dot(const float* __restrict__ nrm, int64_t i, int64_t j)
{
	double d = 0.0;
#pragma unroll
	for (int a = 0; a < D; ++a) { d = d + static_cast<double>(nrm[i * D + a]) * static_cast<double>(nrm[j * D + a]); }
	return d;
}

// the set's positions in point order (the points outside the tree stay NaN, which the fill wrote) and, as the queries of
// the table, in the tree's own order: a wave's queries are Morton neighbours and walk the same nodes (profiles/normals.md:
// half the time of the input order on a scan); who[r] is the point of sorted slot r
template <int D>
__global__ __launch_bounds__(kThreads) void k_orient_positions(Tree t, float* __restrict__ pos, float* __restrict__ queries,
                                                                uint32_t* __restrict__ who)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= t.nf) { return; }
	const float4  p = t.items[i];
	const float   v[3] = {p.x, p.y, p.z};
	const int64_t me = __float_as_uint(p.w);
	who[i] = static_cast<uint32_t>(me);
#pragma unroll
	for (int d = 0; d < D; ++d) {
		pos[me * D + d]    = v[d];
		queries[i * D + d] = v[d];
	}
}

struct State {
	int64_t             n;
	int64_t             slots;    // nf * k: the table has a row per point of the tree, in the tree's order
	int                 k;
	const uint32_t*     who;      // [nf]  the point of a row
	const float*        pos;      // float[n][D]
	float*              normals;  // float[n][D]
	uint8_t*            live;     // [n]
	uint32_t*           link;     // [n]  representative << 1 | parity
	uint32_t*           link2;    // [n]  the hook kernel's output
	unsigned long long* best1;    // [n]  ~bits(a) << 32 | lo of a root's minimum offer
	uint32_t*           best2;    // [n]  its hi
	uint32_t*           ea;       // [nf][k]  ~bits(a)
	int32_t*            ej;       // [nf][k]  the other end, or -1
	uint32_t*           hooked;   // one counter
	uint32_t*           cmin;     // [n]  a root's smallest member
	unsigned long long* ext;      // [n]  a root's extreme member: ~order(coordinate) << 32 | index
	uint32_t*           votes;    // [n][2]  + and - votes relative to the root's sign
	uint8_t*            turn;     // [n]  a root's decision: members with this parity are negated
};

// live points; every vertex its own root
template <int D>
__global__ __launch_bounds__(kThreads) void k_orient_start(State s)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= s.n) { return; }
	bool ok = true, any = false;
#pragma unroll
	for (int d = 0; d < D; ++d) {
		const float v = s.normals[i * D + d];
		ok  = ok && isfinite(s.pos[i * D + d]) && isfinite(v);
		any = any || v != 0.0f;
	}
	s.live[i]          = ok && any ? 1 : 0;
	s.link[i]          = static_cast<uint32_t>(i) << 1;
	s.best1[i]         = kNoOffer;
	s.best2[i]         = kNone;
	s.cmin[i]          = kNone;
	s.ext[i]           = kNoOffer;
	s.votes[2 * i]     = 0;
	s.votes[2 * i + 1] = 0;
	s.turn[i]          = 0;
}

// the table's slots: usable or not, and a
template <int D>
__global__ __launch_bounds__(kThreads) void k_orient_edges(State s, const long long* __restrict__ idx)
{
	const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (e >= s.slots) { return; }
	const int64_t   i = s.who[e / s.k];
	const long long j = idx[e];
	const bool      usable = j >= 0 && j != i && s.live[i] && s.live[j];
	uint32_t        key = 0;
	if (usable) { key = ~__float_as_uint(static_cast<float>(fabs(line_dot<D>(s.normals, i, j)))); }
	s.ea[e] = key;
	s.ej[e] = usable ? static_cast<int32_t>(j) : -1;
}

__global__ __launch_bounds__(kThreads) void k_orient_propose(State s)
{
	const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (e >= s.slots) { return; }
	const int32_t j = s.ej[e];
	if (j < 0) { return; }
	const uint32_t i  = s.who[e / s.k];
	const uint32_t ci = s.link[i] >> 1, cj = s.link[j] >> 1;
	if (ci == cj) {
		s.ej[e] = -1;
		return;
	}
	const uint32_t           lo  = i < static_cast<uint32_t>(j) ? i : static_cast<uint32_t>(j);
	const unsigned long long key = (static_cast<unsigned long long>(s.ea[e]) << 32) | lo;
	lower64(&s.best1[ci], key);
	lower64(&s.best1[cj], key);
}

__global__ __launch_bounds__(kThreads) void k_orient_select(State s)
{
	const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (e >= s.slots) { return; }
	const int32_t j = s.ej[e];
	if (j < 0) { return; }
	const uint32_t           i   = s.who[e / s.k];
	const uint32_t           ci  = s.link[i] >> 1, cj = s.link[j] >> 1;
	const uint32_t           lo  = i < static_cast<uint32_t>(j) ? i : static_cast<uint32_t>(j);
	const uint32_t           hi  = i < static_cast<uint32_t>(j) ? static_cast<uint32_t>(j) : i;
	const unsigned long long key = (static_cast<unsigned long long>(s.ea[e]) << 32) | lo;
	if (s.best1[ci] == key) { lower32(&s.best2[ci], hi); }
	if (s.best1[cj] == key) { lower32(&s.best2[cj], hi); }
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_orient_hook(State s)
{
	const int64_t i  = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	bool          on = false;
	if (i < s.n) {
		uint32_t                 w  = s.link[i];
		const unsigned long long b1 = s.best1[i];
		if ((w >> 1) == i && b1 != kNoOffer) {
			const uint32_t lo = static_cast<uint32_t>(b1), hi = s.best2[i];
			const uint32_t wl = s.link[lo], wh = s.link[hi];
			const bool     mine = (wl >> 1) == i;  // lo is this component's end
			const uint32_t wu = mine ? wl : wh, wv = mine ? wh : wl;
			const uint32_t cv = wv >> 1;
			const bool     mutual = s.best1[cv] == b1 && s.best2[cv] == hi;
			if (!(mutual && i < cv)) {
				const uint32_t flip = line_dot<D>(s.normals, lo, hi) < 0.0 ? 1u : 0u;
				w  = (cv << 1) | ((wu ^ wv ^ flip) & 1u);
				on = true;
			}
		}
		s.link2[i] = w;
	}
	const unsigned long long m = __ballot(on);
	if (m != 0 && (threadIdx.x & 63) == __ffsll(m) - 1) { atomicAdd(s.hooked, static_cast<uint32_t>(__popcll(m))); }
}

__global__ __launch_bounds__(kThreads) void k_orient_jump(State s)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= s.n) { return; }
	s.best1[i] = kNoOffer;
	s.best2[i] = kNone;
	for (;;) {
		const uint32_t w = word_load(&s.link[i]);
		const uint32_t r = w >> 1;
		if (r == i) { break; }
		const uint32_t wr = word_load(&s.link[r]);
		if ((wr >> 1) == r) { break; }  // the parent is a root (roots do not move in this kernel)
		word_store(&s.link[i], (wr & ~1u) | ((w ^ wr) & 1u));
	}
}

enum { kAnchorNone = 0, kAnchorViewpoints = 1, kAnchorDirections = 2 };

// fp32 bits in an order that ascends with the value (-0 = +0)
__device__ inline uint32_t float_order(float v)
{
	const uint32_t b = __float_as_uint(v + 0.0f);
	return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// per component: the smallest member, the extreme member, the votes
template <int D>
__global__ __launch_bounds__(kThreads) void k_orient_collect(State s, int anchor, const float* __restrict__ guides, int64_t num_guides)
{
	const int64_t i     = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	const bool    valid = i < s.n && s.live[i];
	uint32_t      root  = 0;
	int           vote  = 0;
	if (valid) {
		const uint32_t w = s.link[i];
		root = w >> 1;
		lower32(&s.cmin[root], static_cast<uint32_t>(i));
		lower64(&s.ext[root], (static_cast<unsigned long long>(~float_order(s.pos[i * D + D - 1])) << 32) | static_cast<uint32_t>(i));
		if (anchor != kAnchorNone) {
			double sum = 0.0;
#pragma unroll
			for (int d = 0; d < D; ++d) {
				double g;
				if (anchor == kAnchorViewpoints) {
					g = static_cast<double>(guides[(num_guides == 1 ? 0 : i) * D + d]) - static_cast<double>(s.pos[i * D + d]);
				} else {
					g = static_cast<double>(guides[i * D + d]);
				}
				sum = sum + static_cast<double>(s.normals[i * D + d]) * g;
			}
			if (isfinite(sum)) { vote = sum > 0.0 ? 1 : (sum < 0.0 ? -1 : 0); }
			if (w & 1u) { vote = -vote; }  // relative to the root's sign
		}
	}
	if (anchor == kAnchorNone) { return; }
	// a wave whose voters share one root (the common case) adds its counts once
	const unsigned long long voters = __ballot(vote != 0);
	if (voters == 0) { return; }
	const int      src   = __ffsll(voters) - 1;
	const uint32_t first = __shfl(root, src, 64);
	const bool     split = __any(vote != 0 && root != first);
	const unsigned long long plus = __ballot(vote > 0), minus = __ballot(vote < 0);
	if (!split) {
		if ((threadIdx.x & 63) == src) {
			if (plus) { atomicAdd(&s.votes[2 * static_cast<int64_t>(first)], static_cast<uint32_t>(__popcll(plus))); }
			if (minus) { atomicAdd(&s.votes[2 * static_cast<int64_t>(first) + 1], static_cast<uint32_t>(__popcll(minus))); }
		}
	} else if (vote != 0) {
		atomicAdd(&s.votes[2 * static_cast<int64_t>(root) + (vote > 0 ? 0 : 1)], 1u);
	}
}

// per root: S, as the parity whose members are negated
template <int D>
__global__ __launch_bounds__(kThreads) void k_orient_decide(State s)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= s.n || !s.live[i] || (s.link[i] >> 1) != i) { return; }
	const uint32_t c  = s.cmin[i];
	const uint32_t pc = s.link[c] & 1u;  // t = +1 at c
	// the extreme rule
	const uint32_t e  = static_cast<uint32_t>(s.ext[i]);
	const uint32_t te = (s.link[e] & 1u) ^ pc;
	uint32_t       neg = 0;
	bool           seen = false;
#pragma unroll
	for (int d = D - 1; d >= 0; --d) {
		const float v = s.normals[static_cast<int64_t>(e) * D + d];
		if (!seen && v != 0.0f) {
			seen = true;
			neg  = (v < 0.0f ? 1u : 0u) ^ te;
		}
	}
	// the vote, counted relative to the root's sign
	const uint32_t p0 = s.votes[2 * i], p1 = s.votes[2 * i + 1];
	const uint32_t plus = pc ? p1 : p0, minus = pc ? p0 : p1;
	if (minus > plus) { neg = 1; }
	if (plus > minus) { neg = 0; }
	s.turn[i] = static_cast<uint8_t>(neg ^ pc);
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_orient_apply(State s, long long* __restrict__ components)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= s.n) { return; }
	if (!s.live[i]) {
		if (components) { components[i] = -1; }
		return;
	}
	const uint32_t w = s.link[i], root = w >> 1;
	if ((w & 1u) != s.turn[root]) {
		uint32_t* bits = reinterpret_cast<uint32_t*>(s.normals);
#pragma unroll
		for (int d = 0; d < D; ++d) { bits[i * D + d] ^= 0x80000000u; }
	}
	if (components) { components[i] = static_cast<long long>(s.cmin[root]); }
}

template <int D>
void run(const NearestIndex& t, int k, float max_distance, int anchor, const float* guides, int64_t num_guides, float* normals,
         long long* components, hipStream_t st, OrientStats* stats)
{
	const int64_t n = t.n, slots = t.nf * k;
	const dim3    per_point(blocks_for(n)), per_slot(blocks_for(slots)), block(kThreads);
	hipEvent_t    ev[3] = {nullptr, nullptr, nullptr};
	if (stats) {
		for (auto& e : ev) { FI_HIP_TRY(hipEventCreate(&e)); }
		FI_HIP_TRY(hipEventRecord(ev[0], st));
	}

	// the neighbour table: the tree's own points as queries of fi_knn, every buffer on the device
	DevBuf pos, queries, who, dist, idx;
	pos.alloc(sizeof(float) * D * n);
	FI_HIP_TRY(hipMemsetAsync(pos.p, 0xFF, sizeof(float) * D * n, st));  // NaN
	if (t.nf > 0) {
		queries.alloc(sizeof(float) * D * t.nf);
		who.alloc(sizeof(uint32_t) * t.nf);
		dist.alloc(sizeof(float) * slots);
		idx.alloc(sizeof(long long) * slots);
		hipLaunchKernelGGL(k_orient_positions<D>, dim3(blocks_for(t.nf)), block, 0, st, tree_of(t), pos.as<float>(), queries.as<float>(),
		                   who.as<uint32_t>());
		FI_HIP_TRY(hipGetLastError());
		knn_query(t, t.nf, queries.as<float>(), k, max_distance, dist.as<float>(), idx.as<long long>(), FI_DEVICE, st);
		dist.release();
		queries.release();
	}
	if (stats) { FI_HIP_TRY(hipEventRecord(ev[1], st)); }

	DevBuf live, link, link2, best1, best2, ea, ej, hooked, cmin, ext, votes, turn;
	live.alloc(n);
	link.alloc(sizeof(uint32_t) * n);
	link2.alloc(sizeof(uint32_t) * n);
	best1.alloc(sizeof(uint64_t) * n);
	best2.alloc(sizeof(uint32_t) * n);
	if (slots > 0) {
		ea.alloc(sizeof(uint32_t) * slots);
		ej.alloc(sizeof(int32_t) * slots);
	}
	hooked.alloc(sizeof(uint32_t));
	cmin.alloc(sizeof(uint32_t) * n);
	ext.alloc(sizeof(uint64_t) * n);
	votes.alloc(sizeof(uint32_t) * 2 * n);
	turn.alloc(n);
	State s{};
	s.n       = n;
	s.slots   = slots;
	s.k       = k;
	s.who     = who.as<uint32_t>();
	s.pos     = pos.as<float>();
	s.normals = normals;
	s.live    = live.as<uint8_t>();
	s.link    = link.as<uint32_t>();
	s.link2   = link2.as<uint32_t>();
	s.best1   = best1.as<unsigned long long>();
	s.best2   = best2.as<uint32_t>();
	s.ea      = ea.as<uint32_t>();
	s.ej      = ej.as<int32_t>();
	s.hooked  = hooked.as<uint32_t>();
	s.cmin    = cmin.as<uint32_t>();
	s.ext     = ext.as<unsigned long long>();
	s.votes   = votes.as<uint32_t>();
	s.turn    = turn.as<uint8_t>();
	hipLaunchKernelGGL(k_orient_start<D>, per_point, block, 0, st, s);
	if (slots > 0) { hipLaunchKernelGGL(k_orient_edges<D>, per_slot, block, 0, st, s, idx.as<long long>()); }
	FI_HIP_TRY(hipGetLastError());

	int rounds = 0;
	while (slots > 0) {  // (no finite point: no edges)
		FI_REQUIRE(rounds < 64, FI_ERR_STATE, "normal orientation: %d rounds without an end", rounds);
		++rounds;
		FI_HIP_TRY(hipMemsetAsync(s.hooked, 0, sizeof(uint32_t), st));
		hipLaunchKernelGGL(k_orient_propose, per_slot, block, 0, st, s);
		hipLaunchKernelGGL(k_orient_select, per_slot, block, 0, st, s);
		hipLaunchKernelGGL(k_orient_hook<D>, per_point, block, 0, st, s);
		std::swap(s.link, s.link2);
		hipLaunchKernelGGL(k_orient_jump, per_point, block, 0, st, s);
		FI_HIP_TRY(hipGetLastError());
		uint32_t count = 0;
		FI_HIP_TRY(hipMemcpyAsync(&count, s.hooked, sizeof(count), hipMemcpyDeviceToHost, st));
		FI_HIP_TRY(hipStreamSynchronize(st));
		idx.release();  // (read by the edge values only)
		if (count == 0) { break; }
	}

	hipLaunchKernelGGL(k_orient_collect<D>, per_point, block, 0, st, s, anchor, guides, num_guides);
	hipLaunchKernelGGL(k_orient_decide<D>, per_point, block, 0, st, s);
	hipLaunchKernelGGL(k_orient_apply<D>, per_point, block, 0, st, s, components);
	FI_HIP_TRY(hipGetLastError());
	if (stats) {
		FI_HIP_TRY(hipEventRecord(ev[2], st));
		FI_HIP_TRY(hipEventSynchronize(ev[2]));
		float a = 0, b = 0;
		FI_HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
		FI_HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
		stats->rounds           = rounds;
		stats->launches_a_round = 4;
		stats->table_ms         = a;
		stats->propagate_ms     = b;
		for (auto& e : ev) { (void)hipEventDestroy(e); }
	}
	FI_HIP_TRY(hipStreamSynchronize(st));  // the temporaries die here
}

}  // namespace

void orient_normals(const NearestIndex& t, int k, float max_distance, int anchor, const float* guides, int64_t num_guides,
                    float* normals, long long* components, int memory, hipStream_t st, OrientStats* stats)
{
	if (t.n == 0) { return; }
	AllocStream alloc_on(st);
	OrientStats mine;
	if (!stats && test_switch("FI_ORIENT_STATS")) { stats = &mine; }
	stage::Out<float> nrm(normals, t.D * t.n, memory);  // in and out: a stand-in starts as the caller's normals
	if (nrm.host) { stage::upload(nrm.dev, normals, nrm.count, st); }
	stage::Out<long long> comp(components, t.n, memory);
	stage::In<float>      g(anchor == kAnchorNone ? nullptr : guides, num_guides * t.D, memory, st);
	if (t.D == 2) {
		run<2>(t, k, max_distance, anchor, g, num_guides, nrm, comp, st, stats);
	} else {
		run<3>(t, k, max_distance, anchor, g, num_guides, nrm, comp, st, stats);
	}
	nrm.back(st);
	comp.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
	if (stats == &mine) {
		std::fprintf(stderr, "fi_orient_normals: n %lld k %d rounds %d launches/round %d table_ms %.3f propagate_ms %.3f\n",
		             static_cast<long long>(t.n), k, mine.rounds, mine.launches_a_round, mine.table_ms, mine.propagate_ms);
	}
}

}  // namespace fi
