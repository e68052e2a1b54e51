// fi_align.hip -- the rigid motion that most matched pairs of two point clouds agree on: RANSAC over correspondences with an
// exact inlier count.  The coarse alignment from any pose; fi_register.hip's ICP takes the result as its `initial`.
//
// The contract (include/fi_hip.h fi_align_correspondences; tests/align_reference.py is its definition in
// numpy): the live pairs are those with both indices in range and both points finite, in ascending order; hypothesis h draws
// three of them by fi_uniform.h's counter hash, refuses triangles whose edges differ by more than the similarity, and builds
// the rotation from the two triangles' orthonormal frames and the shift from their centroids; everything is fp64 from the
// fp32 coordinates, one rounding per operation (-ffp-contract=off) over + - * / sqrt, every sum in a fixed order; the score
// is an integer count; ties go to the lowest h.  No float atomics: a repeated call returns the same bytes.
//
// How it is found:
//   live pairs k_align_live marks them, prim::select_indices lists them (ascending), the count stays on the device.
//   models     k_align_models: one thread per hypothesis of a batch of 16384 writes (R, t) as 12 doubles, NaN for an invalid
//              one, and a flag; prim::select_indices lists the valid slots -- about one in a hundred passes the edge test, and
//              scoring the rest would waste 99 % of the lanes.
//   score      k_align_score: a LANE OWNS A VALID HYPOTHESIS -- 12 doubles and its count in registers.  A workgroup of 256
//              lanes stages a tile of 256 live pairs in LDS as 6 doubles each and every lane walks the tile: all lanes of a
//              wave read one address per instruction (a broadcast, no bank conflict), so the count needs no cross-lane
//              operation and no atomic in the loop.  The grid is (pair tiles, capped and strided) x (groups of 256 listed
//              slots; the groups past the list leave at once); a workgroup adds its counts with integer atomics.
//   best       k_align_keys and the batch loop: fi_consensus.h, as the draw at the head of a hypothesis; the head's spare word
//              is the batch's valid count.
//   result     k_align_pick recomputes the winner with the same device function; k_align_flags (one thread per input pair),
//              select_indices (the inlier pairs, ascending), k_align_chunks and k_align_finish (fi_treesum.h's fixed-order
//              sum; then the rms, the result).
// One device allocation (fi_arena.h) a call; one read-back a batch and one for the result.
#include "fi_solver_internal.h"
#include "fi_stage.h"
#include "fi_align.h"
#include "fi_consensus.h"
#include "fi_prim.h"
#include "fi_treesum.h"

#include <algorithm>
#include <cmath>

namespace fi {
namespace {

constexpr int kBatch   = 16384;  // FI_ALIGN_BATCH: the hypotheses drawn before the stop rule is asked
constexpr int kTile    = 256;    // the live pairs a workgroup stages at a time
constexpr int kChunk   = treesum::kChunk;  // the inlier pairs a workgroup sums
constexpr int kMaxTile = 512;    // the cap of the score grid's x
static_assert(kBatch == FI_ALIGN_BATCH, "the batch is part of the contract");
static_assert(kBatch % kThreads == 0 && kTile == kThreads && kChunk == kThreads, "one lane per hypothesis, per staged pair, per member");

// what stays on the device between the kernels of a call
struct AlignState {
	consensus::Head head;    // head.live: the live pairs; head.spare: the valid hypotheses of the batch (select_indices writes it)
	uint32_t        count;   // the inlier pairs of the winner (select_indices writes it)
	double          M[12];   // the winner: row r is R[r][0], R[r][1], R[r][2], t[r]
	fi_alignment    out;
};

struct AlignArgs {
	int64_t              m;
	const float*         src;     // float[n_s][3]
	const float*         tgt;     // float[n_t][3]
	const long long*     si;      // [m]
	const long long*     ti;      // [m]
	const unsigned char* lflag;   // uint8[m]: a live pair
	const uint32_t*      pair;    // the live pairs, ascending
	unsigned char*       flag;    // uint8[m]: an inlier of the winner
	const uint32_t*      member;  // the inlier pairs, ascending
	AlignState*          state;
	uint64_t             seed;
	double               sim2;    // (double)similarity squared; 0: no edge test
	double               thr2;    // (double)threshold squared
	double*              hyp;     // double[12][kBatch]: R and t of the batch
	unsigned char*       vflag;   // uint8[kBatch]: a valid hypothesis
	const uint32_t*      slot;    // the valid slots of the batch, ascending
	uint32_t*            counts;  // uint32[kBatch], by slot; zero between batches
	double*              partial; // double[chunks]
};

__device__ inline void load_point(const float* __restrict__ pos, int64_t i, double (&x)[3])
{
#pragma unroll
	for (int a = 0; a < 3; ++a) { x[a] = static_cast<double>(pos[i * 3 + a]); }
}

__device__ inline double squares(const double (&x)[3]) { return (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]; }

__device__ inline void cross(const double (&u)[3], const double (&w)[3], double (&g)[3])
{
	g[0] = u[1] * w[2] - u[2] * w[1];
	g[1] = u[2] * w[0] - u[0] * w[2];
	g[2] = u[0] * w[1] - u[1] * w[0];
}

// the orthonormal frame of the triangle p: e_1 along p_1 - p_0, e_3 along e_1 x (p_2 - p_0), e_2 = e_3 x e_1
__device__ inline bool frame(const double (&p)[3][3], double (&e)[3][3])
{
	double u[3], w[3], g[3];
#pragma unroll
	for (int x = 0; x < 3; ++x) {
		u[x] = p[1][x] - p[0][x];
		w[x] = p[2][x] - p[0][x];
	}
	const double l1 = sqrt(squares(u));
#pragma unroll
	for (int x = 0; x < 3; ++x) { e[0][x] = u[x] / l1; }
	cross(e[0], w, g);
	const double l = sqrt(squares(g));
#pragma unroll
	for (int x = 0; x < 3; ++x) { e[2][x] = g[x] / l; }
	cross(e[2], e[0], e[1]);
	return isfinite(l1) && l1 > 0.0 && isfinite(l) && l > 0.0;
}

// hypothesis h over the live pairs: (R, t) in M, false when it is invalid
__device__ inline bool hypothesis(const AlignArgs& a, uint64_t h, uint32_t live, double (&M)[12])
{
	if (live < 3u) { return false; }
	uint32_t j[3];
	bool     ok = consensus::draw<3>(a.seed, h, live, j);
	double   p[3][3], q[3][3];
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const uint32_t c = a.pair[j[k]];
		load_point(a.src, a.si[c], p[k]);
		load_point(a.tgt, a.ti[c], q[k]);
	}
	if (a.sim2 > 0.0) {
#pragma unroll
		for (int e = 0; e < 3; ++e) {
			const int from = e == 2 ? 1 : 0, to = e == 0 ? 1 : 2;
			double    ds[3], dt[3];
#pragma unroll
			for (int x = 0; x < 3; ++x) {
				ds[x] = p[to][x] - p[from][x];
				dt[x] = q[to][x] - q[from][x];
			}
			const double ls = squares(ds), lt = squares(dt);
			const double lo = ls < lt ? ls : lt, hi = ls < lt ? lt : ls;
			ok              = ok && lo >= a.sim2 * hi;
		}
	}
	double e[3][3], f[3][3];
	ok = frame(p, e) && ok;
	ok = frame(q, f) && ok;
#pragma unroll
	for (int r = 0; r < 3; ++r) {
#pragma unroll
		for (int c = 0; c < 3; ++c) { M[4 * r + c] = (f[0][r] * e[0][c] + f[1][r] * e[1][c]) + f[2][r] * e[2][c]; }
	}
	double cs[3], ct[3];
#pragma unroll
	for (int x = 0; x < 3; ++x) {
		cs[x] = ((p[0][x] + p[1][x]) + p[2][x]) / 3.0;
		ct[x] = ((q[0][x] + q[1][x]) + q[2][x]) / 3.0;
	}
#pragma unroll
	for (int r = 0; r < 3; ++r) { M[4 * r + 3] = ct[r] - ((M[4 * r] * cs[0] + M[4 * r + 1] * cs[1]) + M[4 * r + 2] * cs[2]); }
	return ok;
}

// the squared distance of R x + t to y
__device__ inline double miss(const double (&M)[12], const double (&x)[3], const double (&y)[3])
{
	double d[3];
#pragma unroll
	for (int r = 0; r < 3; ++r) { d[r] = (((M[4 * r] * x[0] + M[4 * r + 1] * x[1]) + M[4 * r + 2] * x[2]) + M[4 * r + 3]) - y[r]; }
	return squares(d);
}

// ---- live pairs, models, score, best ------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_align_live(int64_t m, int64_t ns, int64_t nt, const float* __restrict__ src,
                                                          const float* __restrict__ tgt, const long long* __restrict__ si,
                                                          const long long* __restrict__ ti, unsigned char* __restrict__ lflag)
{
	const int64_t c = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (c >= m) { return; }
	const long long s = si[c], t = ti[c];
	bool            ok = s >= 0 && s < ns && t >= 0 && t < nt;
	if (ok) {
#pragma unroll
		for (int a = 0; a < 3; ++a) { ok = ok && isfinite(src[s * 3 + a]) && isfinite(tgt[t * 3 + a]); }
	}
	lflag[c] = ok ? 1 : 0;
}

// slot t of the batch is hypothesis first + t; the slots behind `count` are invalid
__global__ __launch_bounds__(kThreads) void k_align_models(AlignArgs a, int64_t first, int count)
{
	const int  t = blockIdx.x * kThreads + threadIdx.x;
	double     M[12];
	const bool ok = t < count && hypothesis(a, static_cast<uint64_t>(first + t), a.state->head.live, M);
#pragma unroll
	for (int x = 0; x < 12; ++x) { a.hyp[x * kBatch + t] = ok ? M[x] : NAN; }
	a.vflag[t] = ok ? 1 : 0;
}

// lane t of group blockIdx.y owns the listed slot blockIdx.y * 256 + t; the workgroup walks the tiles blockIdx.x,
// blockIdx.x + gridDim.x, ...  A lane past the list owns a NaN model, and the NaN padding of the last tile counts nothing.
__global__ __launch_bounds__(kThreads) void k_align_score(AlignArgs a)
{
	__shared__ double s[kTile][6];
	const int         t      = threadIdx.x;
	const uint32_t    nvalid = a.state->head.spare;
	const uint32_t    at     = blockIdx.y * kThreads + t;
	if (blockIdx.y * kThreads >= nvalid) { return; }  // (the same for every thread of the workgroup)
	const int64_t  live = a.state->head.live;
	const uint32_t slot = at < nvalid ? a.slot[at] : 0u;
	double         M[12];
#pragma unroll
	for (int x = 0; x < 12; ++x) { M[x] = at < nvalid ? a.hyp[x * kBatch + slot] : NAN; }
	const double thr2  = a.thr2;
	uint32_t     count = 0;
	for (int64_t base = static_cast<int64_t>(blockIdx.x) * kTile; base < live; base += static_cast<int64_t>(gridDim.x) * kTile) {
		__syncthreads();  // (the previous tile has been read)
		if (base + t < live) {
			const uint32_t c  = a.pair[base + t];
			const int64_t  is = a.si[c], it = a.ti[c];
#pragma unroll
			for (int x = 0; x < 3; ++x) {
				s[t][x]     = static_cast<double>(a.src[is * 3 + x]);
				s[t][3 + x] = static_cast<double>(a.tgt[it * 3 + x]);
			}
		} else {
#pragma unroll
			for (int x = 0; x < 6; ++x) { s[t][x] = NAN; }
		}
		__syncthreads();
#pragma unroll 4
		for (int k = 0; k < kTile; ++k) {
			double x[3], y[3];
#pragma unroll
			for (int c = 0; c < 3; ++c) {
				x[c] = s[k][c];
				y[c] = s[k][3 + c];
			}
			count += miss(M, x, y) <= thr2 ? 1u : 0u;
		}
	}
	if (count != 0) { atomicAdd(&a.counts[slot], count); }
}

__global__ __launch_bounds__(kThreads) void k_align_keys(AlignArgs a, int64_t first)
{
	consensus::keep_best(blockIdx.x * kThreads + threadIdx.x, first, a.vflag, a.counts, &a.state->head);
}

// the winner becomes the result's motion: the same function of (seed, h, live pairs), so the same bits
__global__ __launch_bounds__(64) void k_align_pick(AlignArgs a, uint64_t h)
{
	if (threadIdx.x != 0) { return; }
	double M[12];
	hypothesis(a, h, a.state->head.live, M);
#pragma unroll
	for (int x = 0; x < 12; ++x) { a.state->M[x] = M[x]; }
}

// ---- the inliers of the winner, the result ------------------------------------------------------------------------------

__device__ inline double miss_of_pair(const AlignArgs& a, const double (&M)[12], int64_t c)
{
	double x[3], y[3];
	load_point(a.src, a.si[c], x);
	load_point(a.tgt, a.ti[c], y);
	return miss(M, x, y);
}

__global__ __launch_bounds__(kThreads) void k_align_flags(AlignArgs a)
{
	const int64_t c = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (c >= a.m) { return; }
	bool in = false;
	if (a.lflag[c]) {
		double M[12];
#pragma unroll
		for (int x = 0; x < 12; ++x) { M[x] = a.state->M[x]; }
		in = miss_of_pair(a, M, c) <= a.thr2;
	}
	a.flag[c] = in ? 1 : 0;
}

// one workgroup per chunk of 256 consecutive inlier pairs: the block tree of their squared misses; the tail adds 0.0
__global__ __launch_bounds__(kChunk) void k_align_chunks(AlignArgs a)
{
	__shared__ double s[1][kChunk];
	const int64_t     count = a.state->count;
	const int64_t     first = static_cast<int64_t>(blockIdx.x) * kChunk;
	if (first >= count) { return; }  // (the same for every thread of the workgroup)
	const int t    = threadIdx.x;
	double    v[1] = {0.0};
	if (first + t < count) {
		double M[12];
#pragma unroll
		for (int x = 0; x < 12; ++x) { M[x] = a.state->M[x]; }
		v[0] = miss_of_pair(a, M, a.member[first + t]);
	}
	treesum::block_tree<1>(v, s);
	if (t == 0) { a.partial[blockIdx.x] = s[0][0]; }
}

// one wave: the chunk sums in ascending order; the result
__global__ __launch_bounds__(64) void k_align_finish(AlignArgs a)
{
	AlignState&   st    = *a.state;
	const int     lane  = threadIdx.x;
	const int64_t count = st.count;
	double        total[1];
	treesum::ordered_sum<1>(a.partial, 1, (count + kChunk - 1) / kChunk, lane, total);
	if (lane != 0) { return; }
	fi_alignment o{};
	o.found   = 1;
	o.inliers = static_cast<long>(count);
#pragma unroll
	for (int x = 0; x < 12; ++x) { o.transform[x] = st.M[x]; }
	o.transform[15] = 1.0;
	o.rms           = count > 0 ? sqrt(total[0] / static_cast<double>(count)) : 0.0;
	st.out          = o;
}

// ---- the host side ------------------------------------------------------------------------------------------------------

using namespace prim;  // Arena, Scratch, arena_alloc, select_marked, grid
static_assert(kThreads == kGridThreads, "grid() counts work groups of kThreads");

void identity(fi_alignment* out, int64_t m)
{
	*out       = fi_alignment{};
	out->pairs = static_cast<long>(m);
	for (int d = 0; d < 4; ++d) { out->transform[5 * d] = 1.0; }
}

}  // namespace

void align_correspondences(int64_t n_s, const float* source, int64_t n_t, const float* target, int64_t m, const long long* src_index,
                           const long long* tgt_index, const fi_align_options& opt, fi_alignment* out, unsigned char* inliers, int memory)
{
	identity(out, m);
	if (m == 0) { return; }
	hipStream_t   st      = nullptr;
	const int64_t chunks  = (m + kChunk - 1) / kChunk;
	AlignArgs     a{};
	DevBuf        block;
	Scratch       tmp;
	unsigned char* lflag  = nullptr;
	uint32_t *     pair = nullptr, *member = nullptr, *slot = nullptr;
	tmp.bytes = std::max(select_bytes(m), select_bytes(kBatch));
	arena_alloc(block, [&](Arena& ar) {  // (an empty set is not uploaded)
		a.state   = ar.take<AlignState>(1);
		a.hyp     = ar.take<double>(12 * kBatch);
		a.partial = ar.take<double>(chunks);
		a.si      = stage::in(ar, src_index, m, memory, st);
		a.ti      = stage::in(ar, tgt_index, m, memory, st);
		a.counts  = ar.take<uint32_t>(kBatch);
		slot      = ar.take<uint32_t>(kBatch);
		pair      = ar.take<uint32_t>(m);
		member    = ar.take<uint32_t>(m);
		a.src     = stage::in(ar, source, n_s * 3, memory, st);
		a.tgt     = stage::in(ar, target, n_t * 3, memory, st);
		a.vflag   = ar.take<unsigned char>(kBatch);
		lflag     = ar.take<unsigned char>(m);
		a.flag    = stage::work(ar, inliers, m, memory);
		tmp.p     = ar.take<char>(static_cast<int64_t>(tmp.bytes));
	});
	FI_HIP_TRY(hipMemsetAsync(a.counts, 0, sizeof(uint32_t) * kBatch, st));
	FI_HIP_TRY(hipMemsetAsync(a.state, 0, sizeof(AlignState), st));
	a.m      = m;
	a.lflag  = lflag;
	a.pair   = pair;
	a.member = member;
	a.slot   = slot;
	a.seed   = opt.seed;
	const double sim = static_cast<double>(opt.similarity), thr = static_cast<double>(opt.threshold);
	a.sim2   = sim * sim;
	a.thr2   = thr * thr;

	hipLaunchKernelGGL(k_align_live, grid(m), dim3(kThreads), 0, st, m, n_s, n_t, a.src, a.tgt, a.si, a.ti, lflag);
	FI_HIP_TRY(hipGetLastError());
	select_marked(lflag, pair, &a.state->head.live, m, tmp, st);

	const unsigned tiles = static_cast<unsigned>(std::min<int64_t>((m + kTile - 1) / kTile, kMaxTile));
	const consensus::Trials ran = consensus::run_batches(&a.state->head, 3, kBatch, opt.max_trials, opt.confidence, st, [&](int64_t first, int count) {
		hipLaunchKernelGGL(k_align_models, dim3(kBatch / kThreads), dim3(kThreads), 0, st, a, first, count);
		FI_HIP_TRY(hipGetLastError());
		select_marked(a.vflag, slot, &a.state->head.spare, kBatch, tmp, st);
		hipLaunchKernelGGL(k_align_score, dim3(tiles, kBatch / kThreads), dim3(kThreads), 0, st, a);
		hipLaunchKernelGGL(k_align_keys, dim3(kBatch / kThreads), dim3(kThreads), 0, st, a, first);
	});
	out->live   = static_cast<long>(ran.seen.live);
	out->trials = static_cast<long>(ran.T);
	out->valid  = static_cast<long>(ran.spare);
	if (ran.seen.best == 0) {
		if (inliers) {
			if (stage::staged(memory)) {
				std::fill(inliers, inliers + m, static_cast<unsigned char>(0));
			} else {
				FI_HIP_TRY(hipMemsetAsync(inliers, 0, m, st));
				FI_HIP_TRY(hipStreamSynchronize(st));
			}
		}
		return;
	}
	hipLaunchKernelGGL(k_align_pick, dim3(1), dim3(64), 0, st, a, consensus::winner_of(ran.seen.best));
	hipLaunchKernelGGL(k_align_flags, grid(m), dim3(kThreads), 0, st, a);
	FI_HIP_TRY(hipGetLastError());
	select_marked(a.flag, member, &a.state->count, m, tmp, st);
	hipLaunchKernelGGL(k_align_chunks, dim3(static_cast<unsigned>(chunks)), dim3(kChunk), 0, st, a);
	hipLaunchKernelGGL(k_align_finish, dim3(1), dim3(64), 0, st, a);
	FI_HIP_TRY(hipGetLastError());
	AlignState got{};
	FI_HIP_TRY(hipMemcpyAsync(&got, a.state, sizeof(got), hipMemcpyDeviceToHost, st));
	stage::back(inliers, a.flag, m, memory, st);
	FI_HIP_TRY(hipStreamSynchronize(st));
	*out        = got.out;
	out->pairs  = static_cast<long>(m);
	out->live   = static_cast<long>(ran.seen.live);
	out->trials = static_cast<long>(ran.T);
	out->valid  = static_cast<long>(ran.spare);
}

}  // namespace fi
