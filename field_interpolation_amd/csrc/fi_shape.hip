// fi_shape.hip -- the spheres (circles in 2-D) and cylinders of a point cloud: RANSAC with an exact inlier count, algebraic
// least-squares refits, and several shapes peeled off one after the other.  The third user of fi_consensus.h, after
// fi_plane.hip and fi_align.hip: a model, a score kernel and a refit, nothing else.
//
// The contract (include/fi_hip.h fi_shape_fit / fi_shapes_segment; tests/shape_reference.py is its definition
// in numpy): the candidates are the finite, unmasked points (with usable normals where normals are passed) in ascending index;
// hypothesis h draws S of them by fi_uniform.h's counter hash; everything is fp64 from the fp32 inputs, one rounding per
// operation (-ffp-contract=off) over + - * / sqrt, every sum in a fixed order; the score is an integer count; ties go to the
// lowest h.  No float atomics: a repeated call returns the same bytes, whatever the launch shape.
//
// How it is found:
//   candidates k_shape_cand marks them, prim::select_indices lists them (ascending), the count stays on the device.
//   models     k_shape_models: one thread per hypothesis of a batch of 1024 writes the centre (axis point), the axis and the
//              squared band lo2, hi2 -- NaN for an invalid one, which no squared distance lies between.
//   score      k_shape_score: a LANE OWNS A HYPOTHESIS -- 5 doubles for a sphere, 8 for a cylinder, and its count in registers.
//              A workgroup of 256 lanes stages a tile of 256 candidates in LDS as doubles (with their unit normals where the
//              angle test reads them) and every lane walks the tile: all lanes of a wave read one address per instruction (a
//              broadcast, no bank conflict).  The band test is quadratic: no square root in the loop.  The grid is (point
//              tiles, capped and strided) x (4 groups of 256 hypotheses); a lane adds its count with one integer atomic.
//   best       k_shape_keys and the batch loop: fi_consensus.h, as the draw at the head of a hypothesis.
//   refits     k_shape_flags (one thread per point against the current model), select_indices (the members, ascending),
//              k_shape_chunks and k_shape_finish (fi_treesum.h's fixed-order sum; then the Kasa solve, for a cylinder in the
//              frame the Jacobi core gives the members' normals).  The refit loop never returns to the host: a `done` word on
//              the device turns the remaining rounds into no-ops.
// One device allocation (fi_arena.h) a call; per shape one read-back a batch and one for the model.
#include "fi_solver_internal.h"
#include "fi_stage.h"
#include "fi_shape.h"
#include "fi_consensus.h"
#include "fi_jacobi.h"
#include "fi_prim.h"
#include "fi_treesum.h"

#include <algorithm>
#include <cmath>

namespace fi {
namespace {

constexpr int kBatch   = 1024;  // FI_SHAPE_BATCH: the hypotheses scored before the stop rule is asked
constexpr int kTile    = 256;   // the candidates a workgroup stages at a time
constexpr int kChunk   = treesum::kChunk;  // the members a workgroup sums
constexpr int kMaxK    = 10;    // the sums of a chunk pass: at most the 6 + 3 + 1 of a sphere's Kasa pass
constexpr int kMaxTile = 512;   // the cap of the score grid's x (512 x 4 = 2048 workgroups, as the plane unit)
constexpr int kHyp     = 8;     // doubles a hypothesis: c[3], a[3], lo2, hi2
constexpr int kSphere = FI_SHAPE_SPHERE, kCylinder = FI_SHAPE_CYLINDER;
static_assert(kBatch == FI_SHAPE_BATCH, "the batch is part of the contract");
static_assert(kBatch % kThreads == 0 && kTile == kThreads && kChunk == kThreads, "one lane per hypothesis, per staged point, per member");

// S: the points a hypothesis draws
template <int M, int D>
constexpr int sample_of() { return M == kCylinder ? 2 : D + 1; }

// what stays on the device between the kernels of one shape
struct ShapeState {
	consensus::Head head;   // head.live: the candidates; the spare word is not used
	uint32_t        count;  // the members of the current model (select_indices writes it)
	int             done;   // the refits have ended
	int             refits;
	int             pad;
	double          c[3], a[3], r;            // the current model: centre or axis point, axis (a cylinder's), radius
	double          m[3];                     // the members' centroid
	double          na[3], e1[3], e2[3];      // a cylinder's refit: the new axis and the frame across it
	fi_shape_model  out;                      // the final model (k_shape_finish<M, D, 2>)
};

struct ShapeArgs {
	int64_t              n;
	const float*         pos;     // float[n][D]
	const float*         nrm;     // float[n][D] or null
	const unsigned char* cflag;   // uint8[n]: a candidate
	const uint32_t*      cand;    // the candidates, ascending
	unsigned char*       flag;    // uint8[n]: an inlier of the current model
	const uint32_t*      member;  // the inliers, ascending
	ShapeState*          state;
	uint64_t             seed;
	double               thr;         // (double)threshold
	double               rmin, rmax;  // (double)r_min, r_max
	double               mc2;         // (double)normal_cos squared
	int                  angle;       // normal_cos > 0: the angle test is on
	double*              hyp;     // double[kHyp][kBatch]
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

// the products summed over ascending axes
template <int D>
__device__ inline double dot(const double (&a)[D], const double (&b)[D])
{
	double s = a[0] * b[0];
#pragma unroll
	for (int x = 1; x < D; ++x) { s = s + a[x] * b[x]; }
	return s;
}

// normal / length per component; the length (the square root of the squares summed over ascending axes) is returned
template <int D>
__device__ inline double unit_normal(const float* __restrict__ nrm, int64_t i, double (&u)[D])
{
	double v[D];
	load_point<D>(nrm, i, v);
	const double len = sqrt(dot<D>(v, v));
#pragma unroll
	for (int a = 0; a < D; ++a) { u[a] = v[a] / len; }
	return len;
}

// M x = r by Cramer's rule, the cofactors and the determinant in the contract's order; false when the determinant is not
// finite or is 0
template <int D>
__device__ inline bool cramer(const double (&M)[D][D], const double (&r)[D], double (&x)[D])
{
	double det;
	if constexpr (D == 2) {
		det  = M[0][0] * M[1][1] - M[0][1] * M[1][0];
		x[0] = (M[1][1] * r[0] - M[0][1] * r[1]) / det;
		x[1] = (M[0][0] * r[1] - M[1][0] * r[0]) / det;
	} else {
		double C[3][3];
#pragma unroll
		for (int i = 0; i < 3; ++i) {
#pragma unroll
			for (int j = 0; j < 3; ++j) {
				const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
				C[i][j]      = M[i1][j1] * M[i2][j2] - M[i1][j2] * M[i2][j1];
			}
		}
		det = (M[0][0] * C[0][0] + M[0][1] * C[0][1]) + M[0][2] * C[0][2];
#pragma unroll
		for (int j = 0; j < 3; ++j) { x[j] = ((C[0][j] * r[0] + C[1][j] * r[1]) + C[2][j] * r[2]) / det; }
	}
	return isfinite(det) && det != 0.0;
}

// the vector g from the model to x and its squares summed over ascending axes: x - c for a sphere; for a cylinder v = x - q,
// t = v . a, g = v - t a.  The one place this is written: the score, the flags and the result read the same bits
template <int M, int D>
__device__ inline double offset2(const double (&c)[D], const double (&ax)[3], const double (&x)[D], double (&g)[D])
{
#pragma unroll
	for (int k = 0; k < D; ++k) { g[k] = x[k] - c[k]; }
	if constexpr (M == kCylinder) {
		const double t = dot<3>(g, ax);
#pragma unroll
		for (int k = 0; k < 3; ++k) { g[k] = g[k] - t * ax[k]; }
	}
	return dot<D>(g, g);
}

// lo2 <= s <= hi2, both edges in
__device__ inline void band(double r, double thr, double& lo2, double& hi2)
{
	const double d  = r - thr;
	const double lo = d > 0.0 ? d : 0.0;
	const double hi = r + thr;
	lo2             = lo * lo;
	hi2             = hi * hi;
}

// the angle test: (u . g)^2 >= (mc mc)(g . g), false when g . g = 0
template <int D>
__device__ inline bool faces(const double (&u)[D], const double (&g)[D], double s, double mc2)
{
	const double nd = dot<D>(u, g);
	return s > 0.0 && nd * nd >= mc2 * s;
}

// the canonical sign: the component of largest magnitude, the first such axis, is positive
__device__ inline void canonical(const double (&a)[3], double (&out)[3])
{
	double big = a[0];
#pragma unroll
	for (int c = 1; c < 3; ++c) { big = fabs(a[c]) > fabs(big) ? a[c] : big; }
	const bool flip = big < 0.0;
#pragma unroll
	for (int c = 0; c < 3; ++c) { out[c] = flip ? -a[c] : a[c]; }
}

// hypothesis h over m candidates: false when it is invalid
template <int M, int D>
__device__ inline bool hypothesis(const ShapeArgs& a, uint64_t h, uint32_t m, double (&c)[D], double (&ax)[3], double& r)
{
	constexpr int S = sample_of<M, D>();
#pragma unroll
	for (int x = 0; x < 3; ++x) { ax[x] = 0.0; }
	if (m < static_cast<uint32_t>(S)) { return false; }
	uint32_t j[S];
	bool     ok = consensus::draw<S>(a.seed, h, m, j);
	double   p[S][D];
#pragma unroll
	for (int k = 0; k < S; ++k) { load_point<D>(a.pos, a.cand[j[k]], p[k]); }
	if constexpr (M == kSphere) {
		double q[D][D], half[D], cp[D];
#pragma unroll
		for (int k = 0; k < D; ++k) {
#pragma unroll
			for (int x = 0; x < D; ++x) { q[k][x] = p[k + 1][x] - p[0][x]; }
			half[k] = 0.5 * dot<D>(q[k], q[k]);
		}
		ok = cramer<D>(q, half, cp) && ok;
#pragma unroll
		for (int x = 0; x < D; ++x) { c[x] = p[0][x] + cp[x]; }
		r = sqrt(dot<D>(cp, cp));
	} else {
		double n0[3], n1[3], d[3];
		unit_normal<3>(a.nrm, a.cand[j[0]], n0);
		unit_normal<3>(a.nrm, a.cand[j[1]], n1);
		ax[0] = n0[1] * n1[2] - n0[2] * n1[1];
		ax[1] = n0[2] * n1[0] - n0[0] * n1[2];
		ax[2] = n0[0] * n1[1] - n0[1] * n1[0];
		const double len = sqrt(dot<3>(ax, ax));
		ok               = ok && isfinite(len) && len > 0.0;
#pragma unroll
		for (int x = 0; x < 3; ++x) {
			ax[x] = ax[x] / len;
			d[x]  = p[1][x] - p[0][x];
		}
		const double g00 = dot<3>(n0, n0), g01 = dot<3>(n0, n1), g11 = dot<3>(n1, n1), b0 = dot<3>(n0, d), b1 = dot<3>(n1, d);
		const double det = g00 * g11 - g01 * g01;
		ok               = ok && isfinite(det) && det != 0.0;
		const double s   = (b0 * g11 - g01 * b1) / det;
#pragma unroll
		for (int x = 0; x < 3; ++x) { c[x] = p[0][x] + s * n0[x]; }
		r = fabs(s);
	}
	return ok && isfinite(r) && a.rmin <= r && r <= a.rmax;
}

// ---- candidates, models, score, best ------------------------------------------------------------------------------------

// a candidate: every coordinate finite, a usable normal where there are normals, not masked out, not taken by an earlier shape
template <int D>
__global__ __launch_bounds__(kThreads) void k_shape_cand(int64_t n, const float* __restrict__ pos, const float* __restrict__ nrm,
                                                          const unsigned char* __restrict__ mask, const int* __restrict__ labels,
                                                          unsigned char* __restrict__ cflag)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	bool ok = true;
#pragma unroll
	for (int a = 0; a < D; ++a) { ok = ok && isfinite(pos[i * D + a]); }
	if (nrm) {
#pragma unroll
		for (int a = 0; a < D; ++a) { ok = ok && isfinite(nrm[i * D + a]); }
		double       u[D];
		const double len = unit_normal<D>(nrm, i, u);
		ok               = ok && isfinite(len) && len > 0.0;
	}
	if (mask) { ok = ok && mask[i] != 0; }
	if (labels) { ok = ok && labels[i] < 0; }
	cflag[i] = ok ? 1 : 0;
}

// slot t of the batch is hypothesis first + t; the slots behind `count` are invalid
template <int M, int D>
__global__ __launch_bounds__(kThreads) void k_shape_models(ShapeArgs a, int64_t first, int count)
{
	const int t = blockIdx.x * kThreads + threadIdx.x;
	double    c[D], ax[3], r = 0.0, lo2, hi2;
	const bool ok = t < count && hypothesis<M, D>(a, static_cast<uint64_t>(first + t), a.state->head.live, c, ax, r);
	band(r, a.thr, lo2, hi2);
#pragma unroll
	for (int x = 0; x < D; ++x) { a.hyp[x * kBatch + t] = ok ? c[x] : NAN; }
	if constexpr (M == kCylinder) {
#pragma unroll
		for (int x = 0; x < 3; ++x) { a.hyp[(3 + x) * kBatch + t] = ok ? ax[x] : NAN; }
	}
	a.hyp[6 * kBatch + t] = ok ? lo2 : NAN;
	a.hyp[7 * kBatch + t] = ok ? hi2 : NAN;
	a.valid[t]            = ok ? 1 : 0;
}

// lane t of group blockIdx.y owns hypothesis slot blockIdx.y * 256 + t; the workgroup walks the tiles blockIdx.x,
// blockIdx.x + gridDim.x, ...  A NaN band (an invalid slot) and the NaN padding of the last tile count nothing.  NRM: the unit
// normals are staged behind the positions and the angle test is on
template <int M, int D, bool NRM>
__global__ __launch_bounds__(kThreads) void k_shape_score(ShapeArgs a)
{
	constexpr int     WP = D == 3 ? 4 : 2;        // doubles a staged position, and a staged normal
	constexpr int     W  = NRM ? 2 * WP : WP;     // 32 or 64 bytes a point in 3-D
	__shared__ double s[kTile][W];
	const int         t    = threadIdx.x;
	const int         slot = blockIdx.y * kThreads + t;
	const int64_t     m    = a.state->head.live;
	double            c[D], ax[3] = {0.0, 0.0, 0.0};
#pragma unroll
	for (int x = 0; x < D; ++x) { c[x] = a.hyp[x * kBatch + slot]; }
	if constexpr (M == kCylinder) {
#pragma unroll
		for (int x = 0; x < 3; ++x) { ax[x] = a.hyp[(3 + x) * kBatch + slot]; }
	}
	const double lo2   = a.hyp[6 * kBatch + slot];
	const double hi2   = a.hyp[7 * kBatch + slot];
	const double mc2   = a.mc2;
	uint32_t     count = 0;
	for (int64_t base = static_cast<int64_t>(blockIdx.x) * kTile; base < m; base += static_cast<int64_t>(gridDim.x) * kTile) {
		__syncthreads();  // (the previous tile has been read)
		if (base + t < m) {
			const int64_t i = a.cand[base + t];
#pragma unroll
			for (int x = 0; x < D; ++x) { s[t][x] = static_cast<double>(a.pos[i * D + x]); }
			if constexpr (NRM) {
				double u[D];
				unit_normal<D>(a.nrm, i, u);
#pragma unroll
				for (int x = 0; x < D; ++x) { s[t][WP + x] = u[x]; }
			}
		} else {
#pragma unroll
			for (int x = 0; x < D; ++x) { s[t][x] = NAN; }
			if constexpr (NRM) {
#pragma unroll
				for (int x = 0; x < D; ++x) { s[t][WP + x] = NAN; }
			}
		}
		__syncthreads();
#pragma unroll 8
		for (int k = 0; k < kTile; ++k) {
			double x[D], g[D];
#pragma unroll
			for (int e = 0; e < D; ++e) { x[e] = s[k][e]; }
			const double d2 = offset2<M, D>(c, ax, x, g);
			bool         in = lo2 <= d2 && d2 <= hi2;
			if constexpr (NRM) {
				double u[D];
#pragma unroll
				for (int e = 0; e < D; ++e) { u[e] = s[k][WP + e]; }
				in = in && faces<D>(u, g, d2, mc2);
			}
			count += in ? 1u : 0u;
		}
	}
	if (count != 0) { atomicAdd(&a.counts[slot], count); }
}

__global__ __launch_bounds__(kThreads) void k_shape_keys(ShapeArgs a, int64_t first)
{
	consensus::keep_best(blockIdx.x * kThreads + threadIdx.x, first, a.valid, a.counts, &a.state->head);
}

// the winner becomes the current model: the same function of (seed, h, candidates), so the same bits
template <int M, int D>
__global__ __launch_bounds__(64) void k_shape_pick(ShapeArgs a, uint64_t h)
{
	if (threadIdx.x != 0) { return; }
	double c[D], ax[3], r = 0.0;
	hypothesis<M, D>(a, h, a.state->head.live, c, ax, r);
#pragma unroll
	for (int x = 0; x < D; ++x) { a.state->c[x] = c[x]; }
#pragma unroll
	for (int x = 0; x < 3; ++x) { a.state->a[x] = ax[x]; }
	a.state->r = r;
}

// ---- the inliers of the current model, the refits, the result -----------------------------------------------------------

template <int M, int D>
__global__ __launch_bounds__(kThreads) void k_shape_flags(ShapeArgs a, int again)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= a.n || (again && a.state->done)) { return; }
	double c[D], ax[3], x[D], g[D], lo2, hi2;
#pragma unroll
	for (int k = 0; k < D; ++k) { c[k] = a.state->c[k]; }
#pragma unroll
	for (int k = 0; k < 3; ++k) { ax[k] = a.state->a[k]; }
	band(a.state->r, a.thr, lo2, hi2);
	load_point<D>(a.pos, i, x);
	const double d2 = offset2<M, D>(c, ax, x, g);
	bool         in = a.cflag[i] && lo2 <= d2 && d2 <= hi2;
	if (in && a.angle) {
		double u[D];
		unit_normal<D>(a.nrm, i, u);
		in = faces<D>(u, g, d2, a.mc2);
	}
	a.flag[i] = in ? 1 : 0;
}

// PASS 0: the members' coordinates, for a cylinder also the products n_a n_b (a <= b, rows first) of their unit normals;
// PASS 1: the Kasa sums of y = x - m (a cylinder: of (y . e_1, y . e_2)): y_a y_b (a <= b, rows first), y_a w, w = y . y;
// PASS 2: (sqrt(s) - r)^2
template <int M, int D, int PASS>
constexpr int sums_of()
{
	constexpr int F = M == kCylinder ? 2 : D;  // the dimension the Kasa solve runs in
	return PASS == 0 ? (M == kCylinder ? 9 : D) : PASS == 1 ? F * (F + 1) / 2 + F + 1 : 1;
}

template <int F>
__device__ inline void kasa_terms(const double (&y)[F], double* v)
{
	const double w = dot<F>(y, y);
	int          k = 0;
#pragma unroll
	for (int p = 0; p < F; ++p) {
#pragma unroll
		for (int q = p; q < F; ++q) { v[k++] = y[p] * y[q]; }
	}
#pragma unroll
	for (int p = 0; p < F; ++p) { v[k++] = y[p] * w; }
	v[k] = w;
}

// one workgroup per chunk of 256 consecutive members: the block tree of their terms; the tail adds 0.0.  A cylinder's PASS 2
// also leaves the least and the greatest (x - q) . axis of the chunk behind its sum, the axis with its canonical sign
template <int M, int D, int PASS>
__global__ __launch_bounds__(kChunk) void k_shape_chunks(ShapeArgs a)
{
	constexpr int     K = sums_of<M, D, PASS>();
	__shared__ double s[K][kChunk];
	const ShapeState& st    = *a.state;
	const int64_t     count = st.count;
	const int64_t     first = static_cast<int64_t>(blockIdx.x) * kChunk;
	if (first >= count || (PASS != 2 && st.done)) { return; }  // (the same for every thread of the workgroup)
	const int  t    = threadIdx.x;
	const bool have = first + t < count;
	double     v[K], along = 0.0;
#pragma unroll
	for (int k = 0; k < K; ++k) { v[k] = 0.0; }
	if (have) {
		const int64_t i = a.member[first + t];
		double        x[D];
		load_point<D>(a.pos, i, x);
		if constexpr (PASS == 0) {
#pragma unroll
			for (int c = 0; c < D; ++c) { v[c] = x[c]; }
			if constexpr (M == kCylinder) {
				double u[3];
				unit_normal<3>(a.nrm, i, u);
				int k = 3;
#pragma unroll
				for (int p = 0; p < 3; ++p) {
#pragma unroll
					for (int q = p; q < 3; ++q) { v[k++] = u[p] * u[q]; }
				}
			}
		} else if constexpr (PASS == 1) {
			double y[D];
#pragma unroll
			for (int c = 0; c < D; ++c) { y[c] = x[c] - st.m[c]; }
			if constexpr (M == kCylinder) {
				const double f[2] = {dot<3>(y, st.e1), dot<3>(y, st.e2)};
				kasa_terms<2>(f, v);
			} else {
				kasa_terms<D>(y, v);
			}
		} else {
			double c[D], ax[3], g[D];
#pragma unroll
			for (int k = 0; k < D; ++k) { c[k] = st.c[k]; }
#pragma unroll
			for (int k = 0; k < 3; ++k) { ax[k] = st.a[k]; }
			const double e = sqrt(offset2<M, D>(c, ax, x, g)) - st.r;
			v[0]           = e * e;
			if constexpr (M == kCylinder) {
				double d[3], sa[3];
				canonical(ax, sa);
#pragma unroll
				for (int k = 0; k < 3; ++k) { d[k] = x[k] - c[k]; }
				along = dot<3>(d, sa);
			}
		}
	}
	treesum::block_tree<K>(v, s);
	if (t < K) { a.partial[static_cast<int64_t>(blockIdx.x) * kMaxK + t] = s[t][0]; }
	if constexpr (M == kCylinder && PASS == 2) {
		__shared__ double lo[kChunk], hi[kChunk];
		lo[t] = have ? along : INFINITY;
		hi[t] = have ? along : -INFINITY;
		__syncthreads();
		for (int w = kChunk / 2; w > 0; w >>= 1) {
			if (t < w) {
				lo[t] = lo[t + w] < lo[t] ? lo[t + w] : lo[t];
				hi[t] = hi[t + w] > hi[t] ? hi[t + w] : hi[t];
			}
			__syncthreads();
		}
		if (t == 0) {
			a.partial[static_cast<int64_t>(blockIdx.x) * kMaxK + 1] = lo[0];
			a.partial[static_cast<int64_t>(blockIdx.x) * kMaxK + 2] = hi[0];
		}
	}
}

// the Kasa solve over the totals of PASS 1: (sum y y^T) c' = 1/2 sum y w, r = sqrt(c' . c' + sum w / count)
template <int F>
__device__ inline bool kasa_solve(const double* total, double count, double (&cp)[F], double& r)
{
	double A[F][F], rhs[F];
	int    k = 0;
#pragma unroll
	for (int p = 0; p < F; ++p) {
#pragma unroll
		for (int q = p; q < F; ++q) {
			A[p][q] = total[k];
			A[q][p] = total[k];
			++k;
		}
	}
#pragma unroll
	for (int p = 0; p < F; ++p) { rhs[p] = 0.5 * total[k++]; }
	const bool ok = cramer<F>(A, rhs, cp);
	r             = sqrt(dot<F>(cp, cp) + total[k] / count);
	return ok;
}

// one wave: the chunk sums in ascending order; then the centroid and a cylinder's frame (PASS 0), the refitted model (PASS 1)
// or the result (PASS 2)
template <int M, int D, int PASS>
__global__ __launch_bounds__(64) void k_shape_finish(ShapeArgs a)
{
	constexpr int K    = sums_of<M, D, PASS>();
	constexpr int S    = sample_of<M, D>();
	ShapeState&   st   = *a.state;
	const int     lane = threadIdx.x;
	if (PASS != 2 && st.done) { return; }
	const int64_t count = st.count;
	if (PASS == 0 && count < S + 1) {
		if (lane == 0) { st.done = 1; }
		return;
	}
	const int64_t nb = (count + kChunk - 1) / kChunk;
	double        total[K];
	treesum::ordered_sum<K>(a.partial, kMaxK, nb, lane, total);
	double tmin = INFINITY, tmax = -INFINITY;
	if constexpr (M == kCylinder && PASS == 2) {
		// maxima do not depend on the order
		for (int64_t b = lane; b < nb; b += 64) {
			const double lo = a.partial[b * kMaxK + 1], hi = a.partial[b * kMaxK + 2];
			tmin            = lo < tmin ? lo : tmin;
			tmax            = hi > tmax ? hi : tmax;
		}
		for (int o = 32; o > 0; o >>= 1) {
			const double lo = __shfl_xor(tmin, o, 64), hi = __shfl_xor(tmax, o, 64);
			tmin            = lo < tmin ? lo : tmin;
			tmax            = hi > tmax ? hi : tmax;
		}
	}
	if (lane != 0) { return; }
	const double cnt = static_cast<double>(count);
	if constexpr (PASS == 0) {
#pragma unroll
		for (int c = 0; c < D; ++c) { st.m[c] = total[c] / cnt; }
		if constexpr (M == kCylinder) {
			double A[3][3], V[3][3];
			int    k = 3;
#pragma unroll
			for (int p = 0; p < 3; ++p) {
#pragma unroll
				for (int q = p; q < 3; ++q) {
					A[p][q] = total[k];
					A[q][p] = total[k];
					++k;
				}
			}
#pragma unroll
			for (int p = 0; p < 3; ++p) {
#pragma unroll
				for (int q = 0; q < 3; ++q) { V[p][q] = p == q ? 1.0 : 0.0; }
			}
			jacobi::jacobi_sweeps<3>(A, V);
			// the axis: the column of the smallest diagonal entry, the lowest on a tie; not renormalised.  e_1, e_2: the other
			// two in ascending column order
			int    col  = 0;
			double lmin = A[0][0];
#pragma unroll
			for (int c = 1; c < 3; ++c) {
				if (A[c][c] < lmin) {
					lmin = A[c][c];
					col  = c;
				}
			}
			bool finite = true;
#pragma unroll
			for (int c = 0; c < 3; ++c) {
				st.na[c] = col == 0 ? V[c][0] : col == 1 ? V[c][1] : V[c][2];
				st.e1[c] = col == 0 ? V[c][1] : V[c][0];
				st.e2[c] = col == 2 ? V[c][1] : V[c][2];
				finite   = finite && isfinite(V[c][0]) && isfinite(V[c][1]) && isfinite(V[c][2]);
			}
			if (!finite) { st.done = 1; }  // the refit is skipped: the model stays
		}
	} else if constexpr (PASS == 1) {
		double c[D], r;
		bool   ok;
		if constexpr (M == kCylinder) {
			double cp[2];
			ok = kasa_solve<2>(total, cnt, cp, r);
#pragma unroll
			for (int x = 0; x < 3; ++x) { c[x] = (st.m[x] + cp[0] * st.e1[x]) + cp[1] * st.e2[x]; }
		} else {
			double cp[D];
			ok = kasa_solve<D>(total, cnt, cp, r);
#pragma unroll
			for (int x = 0; x < D; ++x) { c[x] = st.m[x] + cp[x]; }
		}
#pragma unroll
		for (int x = 0; x < D; ++x) { ok = ok && isfinite(c[x]); }
		ok = ok && isfinite(r) && a.rmin <= r && r <= a.rmax;
		if (!ok) {
			st.done = 1;  // the refit is skipped: the model stays
			return;
		}
#pragma unroll
		for (int x = 0; x < D; ++x) { st.c[x] = c[x]; }
		if constexpr (M == kCylinder) {
#pragma unroll
			for (int x = 0; x < 3; ++x) { st.a[x] = st.na[x]; }
		}
		st.r      = r;
		st.refits = st.refits + 1;
	} else {
		fi_shape_model o{};
		o.found   = 1;
		o.kind    = M;
		o.refits  = st.refits;
		o.inliers = static_cast<long>(count);
#pragma unroll
		for (int c = 0; c < D; ++c) { o.center[c] = st.c[c]; }
		o.radius = st.r;
		if constexpr (M == kCylinder) {
			canonical(st.a, o.axis);
			if (count > 0) {
				o.extent[0] = tmin;
				o.extent[1] = tmax;
			}
		}
		o.rms  = count > 0 ? sqrt(total[0] / cnt) : 0.0;
		st.out = o;
	}
}

__global__ __launch_bounds__(kThreads) void k_shape_label(int64_t n, const unsigned char* __restrict__ flag, int shape, int* __restrict__ labels)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i < n && flag[i]) { labels[i] = shape; }
}

// ---- the host side ------------------------------------------------------------------------------------------------------

using namespace prim;  // Arena, Scratch, arena_alloc, select_marked, grid
static_assert(kThreads == kGridThreads, "grid() counts work groups of kThreads");

// a call's temporaries; with host buffers also the staged inputs
struct ShapeWork {
	ShapeArgs            a;
	unsigned char*       cflag;
	uint32_t *           cand, *member;
	const unsigned char* mask;
	Scratch              tmp;
};

template <int D>
void lay_out(ShapeWork& w, DevBuf& block, int64_t n, const float* positions, const float* normals, const unsigned char* mask,
             unsigned char* flag, const fi_shape_options& opt, int memory, hipStream_t st)
{
	const int64_t chunks = (n + kChunk - 1) / kChunk;
	w.tmp.bytes = select_bytes(n);
	arena_alloc(block, [&](Arena& ar) {
		w.a.state   = ar.take<ShapeState>(1);
		w.a.hyp     = ar.take<double>(kHyp * kBatch);
		w.a.valid   = ar.take<unsigned char>(kBatch);
		w.a.counts  = ar.take<uint32_t>(kBatch);
		w.a.partial = ar.take<double>(chunks * kMaxK);
		w.cflag     = ar.take<unsigned char>(n);
		w.a.flag    = stage::work(ar, flag, n, memory);
		w.cand      = ar.take<uint32_t>(n);
		w.member    = ar.take<uint32_t>(n);
		w.a.pos     = stage::in(ar, positions, n * D, memory, st);
		w.a.nrm     = stage::in(ar, normals, n * D, memory, st);
		w.mask      = stage::in(ar, mask, n, memory, st);
		w.tmp.p     = ar.take<char>(static_cast<int64_t>(w.tmp.bytes));
	});
	FI_HIP_TRY(hipMemsetAsync(w.a.counts, 0, sizeof(uint32_t) * kBatch, st));
	w.a.n           = n;
	w.a.cflag       = w.cflag;
	w.a.cand        = w.cand;
	w.a.member      = w.member;
	w.a.thr         = static_cast<double>(opt.threshold);
	w.a.rmin        = static_cast<double>(opt.r_min);
	w.a.rmax        = static_cast<double>(opt.r_max);
	const double mc = static_cast<double>(opt.normal_cos);
	w.a.mc2         = mc * mc;
	w.a.angle       = opt.normal_cos > 0.0f ? 1 : 0;
}

// one shape over the candidates (labels: the points an earlier shape took are none); the flags of its inliers stay in a.flag
template <int M, int D>
void fit_one(ShapeWork& w, const fi_shape_options& opt, uint64_t seed, const int* labels, fi_shape_model* model, hipStream_t st)
{
	constexpr int S = sample_of<M, D>();
	ShapeArgs&    a = w.a;
	const int64_t n = a.n;
	a.seed          = seed;
	*model          = fi_shape_model{};
	FI_HIP_TRY(hipMemsetAsync(a.state, 0, sizeof(ShapeState), st));
	hipLaunchKernelGGL(k_shape_cand<D>, grid(n), dim3(kThreads), 0, st, n, a.pos, a.nrm, w.mask, labels, w.cflag);
	FI_HIP_TRY(hipGetLastError());
	select_marked(w.cflag, w.cand, &a.state->head.live, n, w.tmp, st);

	const unsigned tiles = static_cast<unsigned>(std::min<int64_t>((n + kTile - 1) / kTile, kMaxTile));
	const consensus::Trials ran = consensus::run_batches(&a.state->head, S, kBatch, opt.max_trials, opt.confidence, st, [&](int64_t first, int count) {
		const dim3 shape(tiles, (count + kThreads - 1) / kThreads);
		hipLaunchKernelGGL((k_shape_models<M, D>), dim3(kBatch / kThreads), dim3(kThreads), 0, st, a, first, count);
		if (a.angle) {
			hipLaunchKernelGGL((k_shape_score<M, D, true>), shape, dim3(kThreads), 0, st, a);
		} else {
			hipLaunchKernelGGL((k_shape_score<M, D, false>), shape, dim3(kThreads), 0, st, a);
		}
		hipLaunchKernelGGL(k_shape_keys, dim3(kBatch / kThreads), dim3(kThreads), 0, st, a, first);
	});
	model->candidates = static_cast<long>(ran.seen.live);
	model->trials     = static_cast<long>(ran.T);
	if (ran.seen.best == 0) {
		FI_HIP_TRY(hipMemsetAsync(a.flag, 0, n, st));
		return;
	}
	hipLaunchKernelGGL((k_shape_pick<M, D>), dim3(1), dim3(64), 0, st, a, consensus::winner_of(ran.seen.best));
	const dim3 chunks(static_cast<unsigned>((n + kChunk - 1) / kChunk));
	for (int round = 0; round <= opt.refine; ++round) {
		hipLaunchKernelGGL((k_shape_flags<M, D>), grid(n), dim3(kThreads), 0, st, a, round > 0 ? 1 : 0);
		FI_HIP_TRY(hipGetLastError());
		select_marked(a.flag, w.member, &a.state->count, n, w.tmp, st);
		if (round == opt.refine) { break; }
		hipLaunchKernelGGL((k_shape_chunks<M, D, 0>), chunks, dim3(kChunk), 0, st, a);
		hipLaunchKernelGGL((k_shape_finish<M, D, 0>), dim3(1), dim3(64), 0, st, a);
		hipLaunchKernelGGL((k_shape_chunks<M, D, 1>), chunks, dim3(kChunk), 0, st, a);
		hipLaunchKernelGGL((k_shape_finish<M, D, 1>), dim3(1), dim3(64), 0, st, a);
	}
	hipLaunchKernelGGL((k_shape_chunks<M, D, 2>), chunks, dim3(kChunk), 0, st, a);
	hipLaunchKernelGGL((k_shape_finish<M, D, 2>), dim3(1), dim3(64), 0, st, a);
	FI_HIP_TRY(hipGetLastError());
	ShapeState got{};
	FI_HIP_TRY(hipMemcpyAsync(&got, a.state, sizeof(got), hipMemcpyDeviceToHost, st));
	FI_HIP_TRY(hipStreamSynchronize(st));
	*model            = got.out;
	model->candidates = static_cast<long>(ran.seen.live);
	model->trials     = static_cast<long>(ran.T);
}

template <int M, int D>
void fit(int64_t n, const float* positions, const float* normals, const unsigned char* mask, const fi_shape_options& opt, fi_shape_model* model,
         unsigned char* inliers, int memory, hipStream_t st)
{
	ShapeWork w{};
	DevBuf    block;
	lay_out<D>(w, block, n, positions, normals, mask, inliers, opt, memory, st);
	fit_one<M, D>(w, opt, opt.seed, nullptr, model, st);
	stage::back(inliers, w.a.flag, n, memory, st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

template <int M, int D>
void segment(int64_t n, const float* positions, const float* normals, const unsigned char* mask, const fi_shape_options& opt, int max_shapes,
             int64_t min_inliers, int* labels, fi_shape_model* rows, int* num_shapes, int memory, hipStream_t st)
{
	ShapeWork w{};
	DevBuf    block;
	lay_out<D>(w, block, n, positions, normals, mask, nullptr, opt, memory, st);
	stage::Out<int> lab(labels, n, memory);
	FI_HIP_TRY(hipMemsetAsync(lab, 0xFF, sizeof(int) * n, st));  // -1
	for (int p = 0; p < max_shapes; ++p) {
		fi_shape_model got{};
		fit_one<M, D>(w, opt, opt.seed + static_cast<uint64_t>(p), lab, &got, st);
		if (!got.found || got.inliers < min_inliers) { break; }
		hipLaunchKernelGGL(k_shape_label, grid(n), dim3(kThreads), 0, st, n, w.a.flag, p, lab);
		FI_HIP_TRY(hipGetLastError());
		rows[p]     = got;
		*num_shapes = p + 1;
	}
	lab.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

}  // namespace

void shape_fit(int ndim, int64_t n, const float* positions, const float* normals, const unsigned char* mask, const fi_shape_options& opt,
               fi_shape_model* model, unsigned char* inliers, int memory)
{
	*model = fi_shape_model{};
	if (n == 0) { return; }
	hipStream_t st = nullptr;
	if (opt.kind == kCylinder) {
		fit<kCylinder, 3>(n, positions, normals, mask, opt, model, inliers, memory, st);
	} else if (ndim == 2) {
		fit<kSphere, 2>(n, positions, normals, mask, opt, model, inliers, memory, st);
	} else {
		fit<kSphere, 3>(n, positions, normals, mask, opt, model, inliers, memory, st);
	}
}

void shapes_segment(int ndim, int64_t n, const float* positions, const float* normals, const unsigned char* mask, const fi_shape_options& opt,
                    int max_shapes, int64_t min_inliers, int* labels, fi_shape_model* rows, int* num_shapes, int memory)
{
	*num_shapes = 0;
	if (n == 0) { return; }
	hipStream_t st = nullptr;
	if (opt.kind == kCylinder) {
		segment<kCylinder, 3>(n, positions, normals, mask, opt, max_shapes, min_inliers, labels, rows, num_shapes, memory, st);
	} else if (ndim == 2) {
		segment<kSphere, 2>(n, positions, normals, mask, opt, max_shapes, min_inliers, labels, rows, num_shapes, memory, st);
	} else {
		segment<kSphere, 3>(n, positions, normals, mask, opt, max_shapes, min_inliers, labels, rows, num_shapes, memory, st);
	}
}

}  // namespace fi
