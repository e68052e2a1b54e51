// fi_plane.hip -- the dominant hyperplanes of a point cloud: RANSAC with an exact inlier count, least-squares refits, and
// several planes peeled off one after the other.
//
// The contract (include/fi_hip.h fi_plane_fit / fi_planes_segment; tests/plane_reference.py is its definition
// in numpy): the candidates are the finite, unmasked points in ascending index; hypothesis h draws D of them by fi_uniform.h's
// counter hash; everything is fp64 from the fp32 coordinates, one rounding per operation (-ffp-contract=off) over + - * / sqrt,
// every sum in a fixed order; the score is an integer count; ties go to the lowest h.  No float atomics: a repeated call
// returns the same bytes, whatever the launch shape.
//
// How it is found:
//   candidates k_plane_cand marks them, prim::select_indices lists them (ascending), the count stays on the device.
//   models     k_plane_models: one thread per hypothesis of a batch of 1024 writes (n, d), NaN for an invalid one.
//   score      k_plane_score: a LANE OWNS A HYPOTHESIS -- (n, d) and its count in registers.  A workgroup of 256 lanes stages a
//              tile of 256 candidates in LDS as doubles and every lane walks the tile: all lanes of a wave read one address
//              per instruction (a broadcast, no bank conflict), so the count needs no cross-lane operation and no atomic in
//              the loop.  The grid is (point tiles, capped and strided) x (4 groups of 256 hypotheses); a workgroup adds its
//              256 counts with integer atomics: integers add up the same in any order.
//   best       k_plane_keys and the batch loop: fi_consensus.h, as the draw at the head of a hypothesis.
//   refits     k_plane_flags (one thread per point against the current model), select_indices (the members, ascending),
//              k_plane_chunks and k_plane_finish (fi_treesum.h's fixed-order sum; then Jacobi, the sign, the model).  The
//              refit loop never returns to the host: a `done` word on the device turns the remaining rounds into no-ops.
// One device allocation (fi_arena.h) a call; per plane one read-back a batch and one for the model.
#include "fi_solver_internal.h"
#include "fi_stage.h"
#include "fi_plane.h"
#include "fi_consensus.h"
#include "fi_jacobi.h"
#include "fi_prim.h"
#include "fi_treesum.h"

#include <algorithm>
#include <cmath>

namespace fi {
namespace {

constexpr int kBatch   = 1024;  // FI_PLANE_BATCH: the hypotheses scored before the stop rule is asked
constexpr int kTile    = 256;   // the candidates a workgroup stages at a time
constexpr int kChunk   = treesum::kChunk;  // the members a workgroup sums
constexpr int kMaxK    = 6;     // the sums of a chunk pass: D centroid sums, D (D + 1) / 2 moments, or e^2
constexpr int kMaxTile = 512;   // the cap of the score grid's x (Guideline 11: 512 x 4 = 2048 workgroups)
static_assert(kBatch == FI_PLANE_BATCH, "the batch is part of the contract");
static_assert(kBatch % kThreads == 0 && kTile == kThreads && kChunk == kThreads, "one lane per hypothesis, per staged point, per member");

// what stays on the device between the kernels of one plane
struct PlaneState {
	consensus::Head head;   // head.live: the candidates; the spare word is not used
	uint32_t        count;  // the members of the current model (select_indices writes it)
	int             done;   // the refits have ended
	int                refits;
	double             n[3], d;  // the current model
	double             c[3];     // the members' centroid
	fi_plane_model     out;      // the final model (k_plane_finish<D, 2>)
};

struct PlaneArgs {
	int64_t              n;
	const float*         pos;     // float[n][D]
	const unsigned char* cflag;   // uint8[n]: a candidate
	const uint32_t*      cand;    // the candidates, ascending
	unsigned char*       flag;    // uint8[n]: an inlier of the current model
	const uint32_t*      member;  // the inliers, ascending
	PlaneState*          state;
	uint64_t             seed;
	double               axis[3];
	double               lim;     // (min_cos min_cos) (axis . axis); used when constrained
	int                  constrained;
	double               thr;     // (double)threshold
	double*              hyp;     // double[4][kBatch]: n_0, n_1, n_2 (unused in 2-D), d of the batch
	unsigned char*       valid;   // uint8[kBatch]: a valid hypothesis
	uint32_t*            counts;  // uint32[kBatch]; zero between batches
	double*              partial; // double[chunks][kMaxK]
};

template <int D>
__device__ inline void load_point(const float* __restrict__ pos, int64_t i, double (&x)[D])
{
#pragma unroll
	for (int a = 0; a < D; ++a) { x[a] = static_cast<double>(pos[i * D + a]); }
}

// e of the contract: ((n_0 x_0 + n_1 x_1) + n_2 x_2) + d
template <int D>
__device__ inline double residual(const double (&n)[D], double d, const double (&x)[D])
{
	double e = n[0] * x[0] + n[1] * x[1];
	if constexpr (D == 3) { e = e + n[2] * x[2]; }
	return e + d;
}

// hypothesis h over m candidates: false when it is invalid
template <int D>
__device__ inline bool hypothesis(const PlaneArgs& a, uint64_t h, uint32_t m, double (&n)[D], double& d)
{
	if (m < static_cast<uint32_t>(D)) { return false; }
	uint32_t   j[D];
	const bool distinct = consensus::draw<D>(a.seed, h, m, j);
	double     p[D][D];
#pragma unroll
	for (int k = 0; k < D; ++k) { load_point<D>(a.pos, a.cand[j[k]], p[k]); }
	if constexpr (D == 3) {
		double u[3], w[3];
#pragma unroll
		for (int x = 0; x < 3; ++x) {
			u[x] = p[1][x] - p[0][x];
			w[x] = p[2][x] - p[0][x];
		}
		n[0] = u[1] * w[2] - u[2] * w[1];
		n[1] = u[2] * w[0] - u[0] * w[2];
		n[2] = u[0] * w[1] - u[1] * w[0];
	} else {
		const double tx = p[1][0] - p[0][0], ty = p[1][1] - p[0][1];
		n[0]            = -ty;
		n[1]            = tx;
	}
	double l2 = n[0] * n[0];
#pragma unroll
	for (int x = 1; x < D; ++x) { l2 = l2 + n[x] * n[x]; }
	const double len = sqrt(l2);
	bool         ok  = distinct && isfinite(len) && len > 0.0;
#pragma unroll
	for (int x = 0; x < D; ++x) { n[x] = n[x] / len; }
	double s = n[0] * p[0][0];
#pragma unroll
	for (int x = 1; x < D; ++x) { s = s + n[x] * p[0][x]; }
	d = -s;
	if (a.constrained) {
		double t = n[0] * a.axis[0];
#pragma unroll
		for (int x = 1; x < D; ++x) { t = t + n[x] * a.axis[x]; }
		ok = ok && t * t >= a.lim;  // (false for a NaN)
	}
	return ok;
}

// ---- candidates, models, score, best ------------------------------------------------------------------------------------

// a candidate: every coordinate finite, not masked out, not taken by an earlier plane
template <int D>
__global__ __launch_bounds__(kThreads) void k_plane_cand(int64_t n, const float* __restrict__ pos, const unsigned char* __restrict__ mask,
                                                          const int* __restrict__ labels, unsigned char* __restrict__ cflag)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	bool ok = true;
#pragma unroll
	for (int a = 0; a < D; ++a) { ok = ok && isfinite(pos[i * D + a]); }
	if (mask) { ok = ok && mask[i] != 0; }
	if (labels) { ok = ok && labels[i] < 0; }
	cflag[i] = ok ? 1 : 0;
}

// slot t of the batch is hypothesis first + t; the slots behind `count` are invalid
template <int D>
__global__ __launch_bounds__(kThreads) void k_plane_models(PlaneArgs a, int64_t first, int count)
{
	const int t = blockIdx.x * kThreads + threadIdx.x;
	double    n[D], d = 0.0;
	const bool ok = t < count && hypothesis<D>(a, static_cast<uint64_t>(first + t), a.state->head.live, n, d);
#pragma unroll
	for (int x = 0; x < D; ++x) { a.hyp[x * kBatch + t] = ok ? n[x] : NAN; }
	a.hyp[3 * kBatch + t] = ok ? d : NAN;
	a.valid[t]            = ok ? 1 : 0;
}

// lane t of group blockIdx.y owns hypothesis slot blockIdx.y * 256 + t; the workgroup walks the tiles blockIdx.x,
// blockIdx.x + gridDim.x, ...  A NaN model (an invalid slot) and the NaN padding of the last tile count nothing.
template <int D>
__global__ __launch_bounds__(kThreads) void k_plane_score(PlaneArgs a)
{
	constexpr int     W = D == 3 ? 4 : 2;  // doubles a staged point: 32 or 16 bytes, read as one or two aligned pieces
	__shared__ double s[kTile][W];
	const int         t    = threadIdx.x;
	const int         slot = blockIdx.y * kThreads + t;
	const int64_t     m    = a.state->head.live;
	double            n[D];
#pragma unroll
	for (int x = 0; x < D; ++x) { n[x] = a.hyp[x * kBatch + slot]; }
	const double d     = a.hyp[3 * kBatch + slot];
	const double thr   = a.thr;
	uint32_t     count = 0;
	for (int64_t base = static_cast<int64_t>(blockIdx.x) * kTile; base < m; base += static_cast<int64_t>(gridDim.x) * kTile) {
		__syncthreads();  // (the previous tile has been read)
		if (base + t < m) {
			const int64_t i = a.cand[base + t];
#pragma unroll
			for (int x = 0; x < D; ++x) { s[t][x] = static_cast<double>(a.pos[i * D + x]); }
		} else {
#pragma unroll
			for (int x = 0; x < D; ++x) { s[t][x] = NAN; }
		}
		__syncthreads();
#pragma unroll 8
		for (int k = 0; k < kTile; ++k) {
			double x[D];
#pragma unroll
			for (int c = 0; c < D; ++c) { x[c] = s[k][c]; }
			count += fabs(residual<D>(n, d, x)) <= thr ? 1u : 0u;
		}
	}
	if (count != 0) { atomicAdd(&a.counts[slot], count); }
}

__global__ __launch_bounds__(kThreads) void k_plane_keys(PlaneArgs a, int64_t first)
{
	consensus::keep_best(blockIdx.x * kThreads + threadIdx.x, first, a.valid, a.counts, &a.state->head);
}

// the winner becomes the current model: the same function of (seed, h, candidates), so the same bits
template <int D>
__global__ __launch_bounds__(64) void k_plane_pick(PlaneArgs a, uint64_t h)
{
	if (threadIdx.x != 0) { return; }
	double n[D], d = 0.0;
	hypothesis<D>(a, h, a.state->head.live, n, d);
#pragma unroll
	for (int x = 0; x < D; ++x) { a.state->n[x] = n[x]; }
	a.state->d = d;
}

// ---- the inliers of the current model, the refits, the result -----------------------------------------------------------

template <int D>
__global__ __launch_bounds__(kThreads) void k_plane_flags(PlaneArgs a, int again)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= a.n || (again && a.state->done)) { return; }
	double n[D], x[D];
#pragma unroll
	for (int c = 0; c < D; ++c) { n[c] = a.state->n[c]; }
	load_point<D>(a.pos, i, x);
	a.flag[i] = a.cflag[i] && fabs(residual<D>(n, a.state->d, x)) <= a.thr ? 1 : 0;
}

// PASS 0: the members' coordinates; PASS 1: the products (x_a - c_a)(x_b - c_b), a <= b, rows first; PASS 2: e^2
template <int D, int PASS>
constexpr int sums_of() { return PASS == 0 ? D : PASS == 1 ? D * (D + 1) / 2 : 1; }

// one workgroup per chunk of 256 consecutive members: the block tree of their terms; the tail adds 0.0
template <int D, int PASS>
__global__ __launch_bounds__(kChunk) void k_plane_chunks(PlaneArgs a)
{
	constexpr int     K = sums_of<D, PASS>();
	__shared__ double s[K][kChunk];
	const PlaneState& st    = *a.state;
	const int64_t     count = st.count;
	const int64_t     first = static_cast<int64_t>(blockIdx.x) * kChunk;
	if (first >= count || (PASS != 2 && st.done)) { return; }  // (the same for every thread of the workgroup)
	const int t = threadIdx.x;
	double    v[K];
#pragma unroll
	for (int k = 0; k < K; ++k) { v[k] = 0.0; }
	if (first + t < count) {
		double x[D];
		load_point<D>(a.pos, a.member[first + t], x);
		if constexpr (PASS == 0) {
#pragma unroll
			for (int c = 0; c < D; ++c) { v[c] = x[c]; }
		} else if constexpr (PASS == 1) {
			double e[D];
#pragma unroll
			for (int c = 0; c < D; ++c) { e[c] = x[c] - st.c[c]; }
			int k = 0;
#pragma unroll
			for (int p = 0; p < D; ++p) {
#pragma unroll
				for (int q = p; q < D; ++q) { v[k++] = e[p] * e[q]; }
			}
		} else {
			double n[D];
#pragma unroll
			for (int c = 0; c < D; ++c) { n[c] = st.n[c]; }
			const double e = residual<D>(n, st.d, x);
			v[0]           = e * e;
		}
	}
	treesum::block_tree<K>(v, s);
	if (t < K) { a.partial[static_cast<int64_t>(blockIdx.x) * kMaxK + t] = s[t][0]; }
}

// one wave: the chunk sums in ascending order; then the centroid (PASS 0), the refitted model (PASS 1) or the result (PASS 2)
template <int D, int PASS>
__global__ __launch_bounds__(64) void k_plane_finish(PlaneArgs a)
{
	constexpr int K    = sums_of<D, PASS>();
	PlaneState&   st   = *a.state;
	const int     lane = threadIdx.x;
	if (PASS != 2 && st.done) { return; }
	const int64_t count = st.count;
	if (PASS == 0 && count < D) {
		if (lane == 0) { st.done = 1; }
		return;
	}
	const int64_t nb = (count + kChunk - 1) / kChunk;
	double        total[K];
	treesum::ordered_sum<K>(a.partial, kMaxK, nb, lane, total);
	if (lane != 0) { return; }
	if constexpr (PASS == 0) {
#pragma unroll
		for (int c = 0; c < D; ++c) { st.c[c] = total[c] / static_cast<double>(count); }
	} else if constexpr (PASS == 1) {
		double A[D][D], V[D][D];
		int    k = 0;
#pragma unroll
		for (int p = 0; p < D; ++p) {
#pragma unroll
			for (int q = p; q < D; ++q) {
				A[p][q] = total[k];
				A[q][p] = total[k];
				++k;
			}
		}
#pragma unroll
		for (int p = 0; p < D; ++p) {
#pragma unroll
			for (int q = 0; q < D; ++q) { V[p][q] = p == q ? 1.0 : 0.0; }
		}
		jacobi::jacobi_sweeps<D>(A, V);
		// the column of the smallest diagonal entry, the lowest on a tie; not renormalised
		int    col  = 0;
		double lmin = A[0][0];
#pragma unroll
		for (int c = 1; c < D; ++c) {
			if (A[c][c] < lmin) {
				lmin = A[c][c];
				col  = c;
			}
		}
		double n[D];
		bool   finite = true;
#pragma unroll
		for (int c = 0; c < D; ++c) {
			n[c] = V[c][0];
#pragma unroll
			for (int x = 1; x < D; ++x) { n[c] = col == x ? V[c][x] : n[c]; }
			finite = finite && isfinite(n[c]);
		}
		if (!finite) {
			st.done = 1;  // the refit is skipped: the model stays
			return;
		}
		double s = n[0] * st.c[0];
#pragma unroll
		for (int c = 1; c < D; ++c) { s = s + n[c] * st.c[c]; }
#pragma unroll
		for (int c = 0; c < D; ++c) { st.n[c] = n[c]; }
		st.d      = -s;
		st.refits = st.refits + 1;
	} else {
		// the canonical sign: the component of largest magnitude, the first such axis, is positive
		double big = st.n[0];
#pragma unroll
		for (int c = 1; c < D; ++c) { big = fabs(st.n[c]) > fabs(big) ? st.n[c] : big; }
		const bool     flip = big < 0.0;
		fi_plane_model o{};
		o.found   = 1;
		o.refits  = st.refits;
		o.inliers = static_cast<long>(count);
#pragma unroll
		for (int c = 0; c < D; ++c) { o.normal[c] = flip ? -st.n[c] : st.n[c]; }
		o.offset = flip ? -st.d : st.d;
		o.rms    = count > 0 ? sqrt(total[0] / static_cast<double>(count)) : 0.0;
		st.out   = o;
	}
}

__global__ __launch_bounds__(kThreads) void k_plane_label(int64_t n, const unsigned char* __restrict__ flag, int plane, int* __restrict__ labels)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i < n && flag[i]) { labels[i] = plane; }
}

// ---- the host side ------------------------------------------------------------------------------------------------------

using namespace prim;  // Arena, Scratch, arena_alloc, select_marked, grid
static_assert(kThreads == kGridThreads, "grid() counts work groups of kThreads");

// a call's temporaries; with host buffers also the staged inputs
struct PlaneWork {
	PlaneArgs      a;
	unsigned char* cflag;
	uint32_t *     cand, *member;
	const unsigned char* mask;
	Scratch        tmp;
};

template <int D>
void lay_out(PlaneWork& w, DevBuf& block, int64_t n, const float* positions, const unsigned char* mask, unsigned char* flag, int memory,
             hipStream_t st)
{
	const int64_t chunks = (n + kChunk - 1) / kChunk;
	w.tmp.bytes = select_bytes(n);
	arena_alloc(block, [&](Arena& ar) {
		w.a.state   = ar.take<PlaneState>(1);
		w.a.hyp     = ar.take<double>(4 * kBatch);
		w.a.valid   = ar.take<unsigned char>(kBatch);
		w.a.counts  = ar.take<uint32_t>(kBatch);
		w.a.partial = ar.take<double>(chunks * kMaxK);
		w.cflag     = ar.take<unsigned char>(n);
		w.a.flag    = stage::work(ar, flag, n, memory);
		w.cand      = ar.take<uint32_t>(n);
		w.member    = ar.take<uint32_t>(n);
		w.a.pos     = stage::in(ar, positions, n * D, memory, st);
		w.mask      = stage::in(ar, mask, n, memory, st);
		w.tmp.p     = ar.take<char>(static_cast<int64_t>(w.tmp.bytes));
	});
	FI_HIP_TRY(hipMemsetAsync(w.a.counts, 0, sizeof(uint32_t) * kBatch, st));
	w.a.n      = n;
	w.a.cflag  = w.cflag;
	w.a.cand   = w.cand;
	w.a.member = w.member;
}

void constrain(PlaneArgs& a, int D, const fi_plane_options& opt)
{
	a.thr         = static_cast<double>(opt.threshold);
	a.constrained = opt.min_cos > 0.0f ? 1 : 0;
	double aa = 0.0;
	for (int x = 0; x < D; ++x) {
		a.axis[x] = static_cast<double>(opt.axis[x]);
		aa        = x == 0 ? a.axis[0] * a.axis[0] : aa + a.axis[x] * a.axis[x];
	}
	const double mc = static_cast<double>(opt.min_cos);
	a.lim           = (mc * mc) * aa;
}

// one plane over the candidates (labels: the points an earlier plane took are none); the flags of its inliers stay in a.flag
template <int D>
void fit_one(PlaneWork& w, const fi_plane_options& opt, uint64_t seed, const int* labels, fi_plane_model* model, hipStream_t st)
{
	PlaneArgs&    a = w.a;
	const int64_t n = a.n;
	a.seed          = seed;
	*model          = fi_plane_model{};
	FI_HIP_TRY(hipMemsetAsync(a.state, 0, sizeof(PlaneState), st));
	hipLaunchKernelGGL(k_plane_cand<D>, grid(n), dim3(kThreads), 0, st, n, a.pos, w.mask, labels, w.cflag);
	FI_HIP_TRY(hipGetLastError());
	select_marked(w.cflag, w.cand, &a.state->head.live, n, w.tmp, st);

	const unsigned tiles = static_cast<unsigned>(std::min<int64_t>((n + kTile - 1) / kTile, kMaxTile));
	const consensus::Trials ran = consensus::run_batches(&a.state->head, D, kBatch, opt.max_trials, opt.confidence, st, [&](int64_t first, int count) {
		hipLaunchKernelGGL(k_plane_models<D>, dim3(kBatch / kThreads), dim3(kThreads), 0, st, a, first, count);
		hipLaunchKernelGGL(k_plane_score<D>, dim3(tiles, (count + kThreads - 1) / kThreads), dim3(kThreads), 0, st, a);
		hipLaunchKernelGGL(k_plane_keys, dim3(kBatch / kThreads), dim3(kThreads), 0, st, a, first);
	});
	model->candidates = static_cast<long>(ran.seen.live);
	model->trials     = static_cast<long>(ran.T);
	if (ran.seen.best == 0) {
		FI_HIP_TRY(hipMemsetAsync(a.flag, 0, n, st));
		return;
	}
	hipLaunchKernelGGL(k_plane_pick<D>, dim3(1), dim3(64), 0, st, a, consensus::winner_of(ran.seen.best));
	const dim3 chunks(static_cast<unsigned>((n + kChunk - 1) / kChunk));
	for (int round = 0; round <= opt.refine; ++round) {
		hipLaunchKernelGGL(k_plane_flags<D>, grid(n), dim3(kThreads), 0, st, a, round > 0 ? 1 : 0);
		FI_HIP_TRY(hipGetLastError());
		select_marked(a.flag, w.member, &a.state->count, n, w.tmp, st);
		if (round == opt.refine) { break; }
		hipLaunchKernelGGL((k_plane_chunks<D, 0>), chunks, dim3(kChunk), 0, st, a);
		hipLaunchKernelGGL((k_plane_finish<D, 0>), dim3(1), dim3(64), 0, st, a);
		hipLaunchKernelGGL((k_plane_chunks<D, 1>), chunks, dim3(kChunk), 0, st, a);
		hipLaunchKernelGGL((k_plane_finish<D, 1>), dim3(1), dim3(64), 0, st, a);
	}
	hipLaunchKernelGGL((k_plane_chunks<D, 2>), chunks, dim3(kChunk), 0, st, a);
	hipLaunchKernelGGL((k_plane_finish<D, 2>), dim3(1), dim3(64), 0, st, a);
	FI_HIP_TRY(hipGetLastError());
	PlaneState got{};
	FI_HIP_TRY(hipMemcpyAsync(&got, a.state, sizeof(got), hipMemcpyDeviceToHost, st));
	FI_HIP_TRY(hipStreamSynchronize(st));
	*model            = got.out;
	model->candidates = static_cast<long>(ran.seen.live);
	model->trials     = static_cast<long>(ran.T);
}

template <int D>
void fit(int64_t n, const float* positions, const unsigned char* mask, const fi_plane_options& opt, fi_plane_model* model,
         unsigned char* inliers, int memory, hipStream_t st)
{
	PlaneWork  w{};
	DevBuf     block;
	lay_out<D>(w, block, n, positions, mask, inliers, memory, st);
	constrain(w.a, D, opt);
	fit_one<D>(w, opt, opt.seed, nullptr, model, st);
	stage::back(inliers, w.a.flag, n, memory, st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

template <int D>
void segment(int64_t n, const float* positions, const unsigned char* mask, const fi_plane_options& opt, int max_planes, int64_t min_inliers,
             int* labels, fi_plane_model* rows, int* num_planes, int memory, hipStream_t st)
{
	PlaneWork  w{};
	DevBuf     block;
	lay_out<D>(w, block, n, positions, mask, nullptr, memory, st);
	constrain(w.a, D, opt);
	stage::Out<int> lab(labels, n, memory);
	FI_HIP_TRY(hipMemsetAsync(lab, 0xFF, sizeof(int) * n, st));  // -1
	for (int p = 0; p < max_planes; ++p) {
		fi_plane_model got{};
		fit_one<D>(w, opt, opt.seed + static_cast<uint64_t>(p), lab, &got, st);
		if (!got.found || got.inliers < min_inliers) { break; }
		hipLaunchKernelGGL(k_plane_label, grid(n), dim3(kThreads), 0, st, n, w.a.flag, p, lab);
		FI_HIP_TRY(hipGetLastError());
		rows[p]     = got;
		*num_planes = p + 1;
	}
	lab.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

}  // namespace

void plane_fit(int ndim, int64_t n, const float* positions, const unsigned char* mask, const fi_plane_options& opt, fi_plane_model* model,
               unsigned char* inliers, int memory)
{
	*model = fi_plane_model{};
	if (n == 0) { return; }
	hipStream_t st = nullptr;
	if (ndim == 2) {
		fit<2>(n, positions, mask, opt, model, inliers, memory, st);
	} else {
		fit<3>(n, positions, mask, opt, model, inliers, memory, st);
	}
}

void planes_segment(int ndim, int64_t n, const float* positions, const unsigned char* mask, const fi_plane_options& opt, int max_planes,
                    int64_t min_inliers, int* labels, fi_plane_model* rows, int* num_planes, int memory)
{
	*num_planes = 0;
	if (n == 0) { return; }
	hipStream_t st = nullptr;
	if (ndim == 2) {
		segment<2>(n, positions, mask, opt, max_planes, min_inliers, labels, rows, num_planes, memory, st);
	} else {
		segment<3>(n, positions, mask, opt, max_planes, min_inliers, labels, rows, num_planes, memory, st);
	}
}

}  // namespace fi
