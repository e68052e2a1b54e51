// fi_register.hip -- rigid registration of a point cloud to a device mesh or to a point set by iterated closest points: the
// loop around the exact searches of fi_surface.hip and fi_nearest.hip, which stay as they are.
//
// The contract (include/fi_hip.h fi_mesh_register / fi_points_register; tests/register_reference.py is its
// definition in numpy): the transform is a D x D matrix R and a vector t in double; an evaluation moves every source point
// (one fp32 rounding), pairs it with its closest point of the target, forms the rows of the linearised problem about the
// pivot g and sums the normal equations in a fixed order -- a tree per block of 256, the blocks in turn; a step solves them
// by a Cholesky factorisation that fixes the unknowns it cannot see, turns the step into an exact rotation by the Cayley map
// and composes it.  fp64 from the fp32 inputs, one rounding per operation (-ffp-contract=off), no sin / cos / atan.  Nothing
// here depends on the run or the launch shape.
//
// How it is found:
//   bounds     k_reg_bounds: every wave's box of its finite source points by shuffles (a maximum needs no order); k_reg_init,
//              one wave, joins them and writes the state -- R, t, the pivot g0 and its image g -- on the device.
//   evaluate   k_reg_transform writes p; fi::surface_query / fi::nearest_query walk p with FI_DEVICE, untouched; k_reg_pairs,
//              the hot kernel, one thread per source point: the pair's primitive or normal, the rows, the weight, and the
//              block's K sums (3-D: 29) by the contract's tree -- w = 128 and 64 through LDS, eight sums at a time, w <= 32 by
//              shuffles in the first wave.
//   step       k_reg_finish, one wave: lane k adds the block partials of sum k in ascending order (eight loads ahead of the
//              additions they feed); lane 0 then factors, solves, maps, composes and tests the stop rule out of LDS and
//              writes the state -- or, for the last evaluation, the result.  The host reads the state once per step.
// No atomics of any kind; one device allocation for every temporary of a call (fi_arena.h); nothing is kept with a handle.
#include "fi_solver_internal.h"
#include "fi_stage.h"
#include "fi_register.h"
#include "fi_prim.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

namespace fi {
namespace {

constexpr int kPlane = FI_REGISTER_PLANE, kPoint = FI_REGISTER_POINT;
constexpr int kMesh = 0, kSet = 1;

constexpr int unknowns(int D) { return D == 3 ? 6 : 3; }
constexpr int sums_of(int D) { return unknowns(D) * (unknowns(D) + 1) / 2 + unknowns(D) + 2; }  // M's upper triangle, b, S_w, S

// what a call keeps on the device between its kernels
struct RegState {
	double R[9], t[3];   // R row-major, D x D in the first D * D entries
	double g0[3], g[3];  // the pivot and its image under (R, t)
	double last_rotation, last_translation;
	int    iterations, converged, fixed_mask;
	int    stop;         // the loop ends: converged, or nothing counted, or no finite source point
	int    any_finite;
};

struct Initial {
	double m[16];  // (D + 1) x (D + 1) row-major
};

// ((R[a][0] x0 + R[a][1] x1) + R[a][2] x2) + t[a]
template <int D>
__device__ inline double affine_row(const double* R, const double* t, int a, const double* x)
{
	double s = R[a * D] * x[0] + R[a * D + 1] * x[1];
	if constexpr (D == 3) { s = s + R[a * D + 2] * x[2]; }
	return s + t[a];
}

// ---- bounds and the state ---------------------------------------------------------------------------------------------

// part[w][0 .. D): the smallest, part[w][D .. 2 D): the largest coordinates of the finite points wave w of the grid met
// (+inf / -inf: none); the grid strides over the points
template <int D>
__global__ __launch_bounds__(kThreads) void k_reg_bounds(int64_t n, const float* __restrict__ src, float* __restrict__ part)
{
	float lo[D], hi[D];
#pragma unroll
	for (int d = 0; d < D; ++d) {
		lo[d] = INFINITY;
		hi[d] = -INFINITY;
	}
	const int64_t step = static_cast<int64_t>(gridDim.x) * kThreads;
	for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += step) {
		float x[D];
		bool  ok = true;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			x[d] = src[i * D + d];
			ok   = ok && isfinite(x[d]);
		}
		if (ok) {
#pragma unroll
			for (int d = 0; d < D; ++d) {
				lo[d] = fminf(lo[d], x[d]);
				hi[d] = fmaxf(hi[d], x[d]);
			}
		}
	}
#pragma unroll
	for (int d = 0; d < D; ++d) {
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) {
			lo[d] = fminf(lo[d], __shfl_xor(lo[d], o, 64));
			hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], o, 64));
		}
	}
	if ((threadIdx.x & 63) == 0) {
		const int64_t w = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) >> 6;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			part[w * 2 * D + d]     = lo[d];
			part[w * 2 * D + D + d] = hi[d];
		}
	}
}

// one wave: the box of nw waves, the pivot, the start (launched with 64 threads)
template <int D>
__global__ __launch_bounds__(64) void k_reg_init(int64_t nw, const float* __restrict__ part, Initial start, RegState* __restrict__ state)
{
	float lo[D], hi[D];
#pragma unroll
	for (int d = 0; d < D; ++d) {
		lo[d] = INFINITY;
		hi[d] = -INFINITY;
	}
	for (int64_t w = threadIdx.x; w < nw; w += 64) {
#pragma unroll
		for (int d = 0; d < D; ++d) {
			lo[d] = fminf(lo[d], part[w * 2 * D + d]);
			hi[d] = fmaxf(hi[d], part[w * 2 * D + D + d]);
		}
	}
#pragma unroll
	for (int d = 0; d < D; ++d) {
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) {
			lo[d] = fminf(lo[d], __shfl_xor(lo[d], o, 64));
			hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], o, 64));
		}
	}
	if (threadIdx.x != 0) { return; }
	RegState s;
	const bool any = lo[0] <= hi[0];
#pragma unroll
	for (int k = 0; k < 9; ++k) { s.R[k] = 0.0; }
#pragma unroll
	for (int a = 0; a < 3; ++a) { s.t[a] = s.g0[a] = s.g[a] = 0.0; }
#pragma unroll
	for (int a = 0; a < D; ++a) {
#pragma unroll
		for (int b = 0; b < D; ++b) { s.R[a * D + b] = start.m[a * (D + 1) + b]; }
		s.t[a] = start.m[a * (D + 1) + D];
		if (any) { s.g0[a] = 0.5 * (static_cast<double>(lo[a]) + static_cast<double>(hi[a])) + 0.0; }  // (+ 0.0: a zero pivot is +0)
	}
#pragma unroll
	for (int a = 0; a < D; ++a) { s.g[a] = affine_row<D>(s.R, s.t, a, s.g0); }
	s.last_rotation = s.last_translation = 0.0;
	s.iterations = s.converged = s.fixed_mask = s.stop = 0;
	s.any_finite = any ? 1 : 0;
	*state       = s;
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_reg_transform(int64_t n, const float* __restrict__ src, const RegState* __restrict__ state,
                                                             float* __restrict__ p)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	double x[D];
#pragma unroll
	for (int d = 0; d < D; ++d) { x[d] = static_cast<double>(src[i * D + d]); }
#pragma unroll
	for (int a = 0; a < D; ++a) { p[i * D + a] = static_cast<float>(affine_row<D>(state->R, state->t, a, x)); }
}

// a point set's points in the order the caller gave them: the search structure keeps the finite ones sorted, each with its
// index (a non-finite point is never nearest, so its slot is never read)
template <int D>
__global__ __launch_bounds__(kThreads) void k_reg_unsort(int64_t nf, int64_t m, const float4* __restrict__ items, float* __restrict__ out)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= nf) { return; }
	const float4  q = items[i];
	const int64_t j = __float_as_uint(q.w);
	if (j >= m) { return; }
	out[j * D] = q.x;
	out[j * D + 1] = q.y;
	if constexpr (D == 3) { out[j * D + 2] = q.z; }
}

// ---- the pairs --------------------------------------------------------------------------------------------------------

struct PairArgs {
	int64_t          n;
	const float*     p;        // float[n][D]: the transformed points
	const float*     dist;     // float[n]: the pair's distance
	const long long* prim;     // long long[n]: the mesh's primitive / the set's point
	const float*     closest;  // float[n][D]: the closest point on the mesh (kMesh)
	const int*       idx;      // the mesh's indices and positions (kMesh, kPlane)
	const float*     pos;
	const float*     tpos;     // the set's points in the caller's order (kSet)
	const float*     tnrm;     // the set's normals (kSet, kPlane)
	const RegState*  state;
	int              loss;
	double           sc;       // scale * tuning
	double*          partial;  // double[blocks][K]
	uint64_t*        count;    // uint64[blocks]: counted | beyond << 16 | invalid << 32 | degenerate << 48
};

// w of the contract from rho
__device__ inline double loss_weight(int loss, double sc, double rho)
{
	if (loss == FI_LOSS_NONE) { return 1.0; }
	const double u = rho / sc;
	if (loss == FI_LOSS_HUBER) { return u <= 1.0 ? 1.0 : 1.0 / u; }
	if (loss == FI_LOSS_CAUCHY) { return 1.0 / (1.0 + u * u); }
	const double t = 1.0 - u * u;
	return u < 1.0 ? t * t : 0.0;
}

constexpr int kBatch = 8;  // sums that cross the waves through LDS at a time

template <int D, int MODE, int TARGET>
__global__ __launch_bounds__(kThreads) void k_reg_pairs(PairArgs a)
{
	constexpr int U = unknowns(D), K = sums_of(D), ROWS = MODE == kPlane ? 1 : D;
	__shared__ double   lds[kBatch][kThreads / 2];
	__shared__ uint32_t tally[kThreads / 64][4];
	const int     t = threadIdx.x;
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + t;
	double        x[K];
#pragma unroll
	for (int k = 0; k < K; ++k) { x[k] = 0.0; }
	bool counted = false, beyond = false, invalid = false, degenerate = false;
	if (i < a.n) {
		const float d = a.dist[i];
		if (isnan(d)) {
			invalid = true;
		} else if (!isfinite(d)) {
			beyond = true;
		} else {
			const int64_t j = a.prim[i];
			double        nrm[D];
			bool          good = true;
			if constexpr (MODE == kPlane) {
				double len;
				if constexpr (TARGET == kMesh) {
					double q[D][D];
#pragma unroll
					for (int k = 0; k < D; ++k) {
						const int64_t v = a.idx[j * D + k];
#pragma unroll
						for (int c = 0; c < D; ++c) { q[k][c] = static_cast<double>(a.pos[v * D + c]); }
					}
					if constexpr (D == 3) {
						double e[3], f[3];
#pragma unroll
						for (int c = 0; c < 3; ++c) {
							e[c] = q[1][c] - q[0][c];
							f[c] = q[2][c] - q[0][c];
						}
						nrm[0] = e[1] * f[2] - e[2] * f[1];
						nrm[1] = e[2] * f[0] - e[0] * f[2];
						nrm[2] = e[0] * f[1] - e[1] * f[0];
						len    = sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
					} else {
						const double ex = q[1][0] - q[0][0], ey = q[1][1] - q[0][1];
						nrm[0] = ey;
						nrm[1] = -ex;
						len    = sqrt(ex * ex + ey * ey);
					}
				} else {
#pragma unroll
					for (int c = 0; c < D; ++c) { nrm[c] = static_cast<double>(a.tnrm[j * D + c]); }
					double l2 = nrm[0] * nrm[0] + nrm[1] * nrm[1];
					if constexpr (D == 3) { l2 = l2 + nrm[2] * nrm[2]; }
					len = sqrt(l2);
				}
				good = isfinite(len) && len != 0.0;
#pragma unroll
				for (int c = 0; c < D; ++c) { nrm[c] = nrm[c] / len; }
			}
			if (!good) {
				degenerate = true;
			} else {
				counted = true;
				double u[D], e[D];
#pragma unroll
				for (int c = 0; c < D; ++c) {
					const double pc = static_cast<double>(a.p[i * D + c]);
					const double cc = static_cast<double>(TARGET == kMesh ? a.closest[i * D + c] : a.tpos[j * D + c]);
					u[c]            = pc - a.state->g[c];
					e[c]            = pc - cc;
				}
				double J[ROWS][U], r[ROWS], rho;
				if constexpr (MODE == kPlane) {
					if constexpr (D == 3) {
						r[0]    = (nrm[0] * e[0] + nrm[1] * e[1]) + nrm[2] * e[2];
						J[0][0] = u[1] * nrm[2] - u[2] * nrm[1];
						J[0][1] = u[2] * nrm[0] - u[0] * nrm[2];
						J[0][2] = u[0] * nrm[1] - u[1] * nrm[0];
						J[0][3] = nrm[0];
						J[0][4] = nrm[1];
						J[0][5] = nrm[2];
					} else {
						r[0]    = nrm[0] * e[0] + nrm[1] * e[1];
						J[0][0] = u[0] * nrm[1] - u[1] * nrm[0];
						J[0][1] = nrm[0];
						J[0][2] = nrm[1];
					}
					rho = fabs(r[0]);
				} else {
#pragma unroll
					for (int q = 0; q < ROWS; ++q) {
						r[q] = e[q];
#pragma unroll
						for (int k = 0; k < U; ++k) { J[q][k] = 0.0; }
					}
					if constexpr (D == 3) {
						J[0][1] = u[2], J[0][2] = -u[1], J[0][3] = 1.0;
						J[1][0] = -u[2], J[1][2] = u[0], J[1][4] = 1.0;
						J[2][0] = u[1], J[2][1] = -u[0], J[2][5] = 1.0;
						rho = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
					} else {
						J[0][0] = -u[1], J[0][1] = 1.0;
						J[1][0] = u[0], J[1][2] = 1.0;
						rho = sqrt(e[0] * e[0] + e[1] * e[1]);
					}
				}
				const double w = loss_weight(a.loss, a.sc, rho);
				int          k = 0;
#pragma unroll
				for (int c = 0; c < U; ++c) {
#pragma unroll
					for (int b = c; b < U; ++b) {
						double s = J[0][c] * J[0][b];
#pragma unroll
						for (int q = 1; q < ROWS; ++q) { s = s + J[q][c] * J[q][b]; }
						x[k++] = w * s;
					}
				}
#pragma unroll
				for (int c = 0; c < U; ++c) {
					double s = J[0][c] * r[0];
#pragma unroll
					for (int q = 1; q < ROWS; ++q) { s = s + J[q][c] * r[q]; }
					x[k++] = w * s;
				}
				double s = r[0] * r[0];
#pragma unroll
				for (int q = 1; q < ROWS; ++q) { s = s + r[q] * r[q]; }
				x[k++] = w * s;
				x[k++] = s;
			}
		}
	}
	// the counts: every wave's by ballots, the four waves' by thread 0
	const uint32_t c0 = __popcll(__ballot(counted)), c1 = __popcll(__ballot(beyond)), c2 = __popcll(__ballot(invalid)),
	               c3 = __popcll(__ballot(degenerate));
	if ((t & 63) == 0) {
		tally[t >> 6][0] = c0;
		tally[t >> 6][1] = c1;
		tally[t >> 6][2] = c2;
		tally[t >> 6][3] = c3;
	}
	// the tree s[t] += s[t + w]: w = 128 and w = 64 through LDS ...
#pragma unroll
	for (int b0 = 0; b0 < K; b0 += kBatch) {
		__syncthreads();
		if (t >= kThreads / 2) {
#pragma unroll
			for (int k = b0; k < b0 + kBatch && k < K; ++k) { lds[k - b0][t - kThreads / 2] = x[k]; }
		}
		__syncthreads();
		if (t < kThreads / 2) {
#pragma unroll
			for (int k = b0; k < b0 + kBatch && k < K; ++k) { x[k] = x[k] + lds[k - b0][t]; }
		}
		__syncthreads();
		if (t >= 64 && t < 128) {
#pragma unroll
			for (int k = b0; k < b0 + kBatch && k < K; ++k) { lds[k - b0][t - 64] = x[k]; }
		}
		__syncthreads();
		if (t < 64) {
#pragma unroll
			for (int k = b0; k < b0 + kBatch && k < K; ++k) { x[k] = x[k] + lds[k - b0][t]; }
		}
	}
	if (t >= 64) { return; }
	// ... and w = 32 .. 1 inside the first wave (lane t of the step reads lane t + w; only lanes below w are read again)
#pragma unroll
	for (int k = 0; k < K; ++k) {
#pragma unroll
		for (int w = 32; w > 0; w >>= 1) { x[k] = x[k] + __shfl_down(x[k], w, 64); }
	}
	if (t == 0) {
		double* out = a.partial + static_cast<int64_t>(blockIdx.x) * K;
#pragma unroll
		for (int k = 0; k < K; ++k) { out[k] = x[k]; }
		uint64_t c = 0;
#pragma unroll
		for (int w = 0; w < kThreads / 64; ++w) {
			c += static_cast<uint64_t>(tally[w][0]) | static_cast<uint64_t>(tally[w][1]) << 16 | static_cast<uint64_t>(tally[w][2]) << 32 |
			     static_cast<uint64_t>(tally[w][3]) << 48;
		}
		a.count[blockIdx.x] = c;
	}
}

// ---- the step ---------------------------------------------------------------------------------------------------------

// the Cayley map of the contract: R_d (D x D, row-major) from the rotation unknowns
template <int D>
__device__ inline void cayley(const double* omega, double* Rd)
{
	if constexpr (D == 2) {
		const double a = 0.5 * omega[0], a2 = a * a, den = 1.0 + a2;
		const double c = (1.0 - a2) / den, s = (2.0 * a) / den;
		Rd[0] = c, Rd[1] = -s, Rd[2] = s, Rd[3] = c;
	} else {
		const double v0 = 0.5 * omega[0], v1 = 0.5 * omega[1], v2 = 0.5 * omega[2];
		const double q = (v0 * v0 + v1 * v1) + v2 * v2, den = 1.0 + q, c0 = 1.0 - q;
		Rd[0] = (c0 + 2.0 * (v0 * v0)) / den;
		Rd[1] = (2.0 * (v0 * v1) - 2.0 * v2) / den;
		Rd[2] = (2.0 * (v0 * v2) + 2.0 * v1) / den;
		Rd[3] = (2.0 * (v0 * v1) + 2.0 * v2) / den;
		Rd[4] = (c0 + 2.0 * (v1 * v1)) / den;
		Rd[5] = (2.0 * (v1 * v2) - 2.0 * v0) / den;
		Rd[6] = (2.0 * (v0 * v2) - 2.0 * v1) / den;
		Rd[7] = (2.0 * (v1 * v2) + 2.0 * v0) / den;
		Rd[8] = (c0 + 2.0 * (v2 * v2)) / den;
	}
}

// One wave (launched with 64 threads).  The sums of nb blocks, then by lane 0: final_eval == 0 a step of the loop into
// *state; else the figures of the last evaluation and the transform into *out.  The small matrices live in LDS, where a
// data-dependent index costs nothing.
template <int D>
__global__ __launch_bounds__(64) void k_reg_finish(int64_t n, int64_t nb, int mode, int final_eval, double rtol, double ttol,
                                                    const double* __restrict__ partial, const uint64_t* __restrict__ count,
                                                    RegState* __restrict__ state, fi_registration* __restrict__ out)
{
	constexpr int U = unknowns(D), K = sums_of(D), NR = D == 3 ? 3 : 1;
	__shared__ double sums[K], M[U][U], L[U][U], y[U], delta[U], Rd[D * D], Rn[D * D], tn[D];
	__shared__ int    fixed[U];
	const int lane = threadIdx.x;
	if (lane < K) {
		const double* q = partial + lane;
		double        s = 0.0;
		int64_t       j = 0;
		// (eight blocks' partials are loaded before the first of them is added: the additions stay in order, the loads overlap)
		for (; j + 8 <= nb; j += 8) {
			const double a0 = q[j * K], a1 = q[(j + 1) * K], a2 = q[(j + 2) * K], a3 = q[(j + 3) * K], a4 = q[(j + 4) * K],
			             a5 = q[(j + 5) * K], a6 = q[(j + 6) * K], a7 = q[(j + 7) * K];
			s = s + a0;
			s = s + a1;
			s = s + a2;
			s = s + a3;
			s = s + a4;
			s = s + a5;
			s = s + a6;
			s = s + a7;
		}
		for (; j < nb; ++j) { s = s + q[j * K]; }
		sums[lane] = s;
	}
	uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
	for (int64_t j = lane; j < nb; j += 64) {
		const uint64_t c = count[j];
		c0 += c & 0xFFFFu;
		c1 += (c >> 16) & 0xFFFFu;
		c2 += (c >> 32) & 0xFFFFu;
		c3 += c >> 48;
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		c0 += __shfl_xor(c0, o, 64);
		c1 += __shfl_xor(c1, o, 64);
		c2 += __shfl_xor(c2, o, 64);
		c3 += __shfl_xor(c3, o, 64);
	}
	__syncthreads();
	if (lane != 0) { return; }
	if (final_eval) {
		fi_registration r;
		for (int k = 0; k < 16; ++k) { r.transform[k] = 0.0; }
		for (int a = 0; a < D; ++a) {
			for (int b = 0; b < D; ++b) { r.transform[a * (D + 1) + b] = state->R[a * D + b]; }
			r.transform[a * (D + 1) + D] = state->t[a];
		}
		r.transform[D * (D + 1) + D] = 1.0;
		r.iterations       = state->iterations;
		r.converged        = state->converged;
		r.fixed_mask       = state->fixed_mask;
		r.reserved         = 0;
		r.queries          = n;
		r.counted          = static_cast<long long>(c0);
		r.beyond           = static_cast<long long>(c1);
		r.invalid          = static_cast<long long>(c2);
		r.degenerate       = static_cast<long long>(c3);
		r.rms              = 0.0;
		r.weighted_rms     = 0.0;
		r.last_rotation    = state->last_rotation;
		r.last_translation = state->last_translation;
		if (c0 > 0) {
			const double rows = static_cast<double>(mode == kPlane ? c0 : D * c0);
			r.weighted_rms    = sqrt(sums[K - 2] / rows);
			r.rms             = sqrt(sums[K - 1] / rows);
		}
		*out = r;
		return;
	}
	if (!state->any_finite || c0 == 0) {
		state->stop = 1;
		return;
	}
	// M (its upper triangle, mirrored) and b
	{
		int k = 0;
		for (int a = 0; a < U; ++a) {
			for (int b = a; b < U; ++b) { M[a][b] = M[b][a] = sums[k++]; }
		}
	}
	const double* rhs = sums + U * (U + 1) / 2;
	double        top = M[0][0];
	for (int j = 1; j < U; ++j) { top = M[j][j] > top ? M[j][j] : top; }
	const double lim  = 1e-12 * top;
	int          mask = 0;
	for (int j = 0; j < U; ++j) {
		double d = M[j][j];
		for (int k = 0; k < j; ++k) {
			if (!fixed[k]) { d = d - L[j][k] * L[j][k]; }
		}
		fixed[j] = !(d > lim);
		delta[j] = 0.0;
		if (fixed[j]) {
			mask |= 1 << j;
			continue;
		}
		L[j][j] = sqrt(d);
		for (int i = j + 1; i < U; ++i) {
			double s = M[j][i];
			for (int k = 0; k < j; ++k) {
				if (!fixed[k]) { s = s - L[i][k] * L[j][k]; }
			}
			L[i][j] = s / L[j][j];
		}
	}
	for (int j = 0; j < U; ++j) {
		if (fixed[j]) { continue; }
		double s = -rhs[j];
		for (int k = 0; k < j; ++k) {
			if (!fixed[k]) { s = s - L[j][k] * y[k]; }
		}
		y[j] = s / L[j][j];
	}
	for (int j = U - 1; j >= 0; --j) {
		if (fixed[j]) { continue; }
		double s = y[j];
		for (int k = U - 1; k > j; --k) {
			if (!fixed[k]) { s = s - L[k][j] * delta[k]; }
		}
		delta[j] = s / L[j][j];
	}
	// the update: t <- (R_d (t - g) + g) + tau, R <- R_d R
	cayley<D>(delta, Rd);
	for (int a = 0; a < D; ++a) {
		double s = Rd[a * D] * (state->t[0] - state->g[0]) + Rd[a * D + 1] * (state->t[1] - state->g[1]);
		if (D == 3) { s = s + Rd[a * D + 2] * (state->t[2] - state->g[2]); }
		tn[a] = (s + state->g[a]) + delta[NR + a];
		for (int b = 0; b < D; ++b) {
			double m = Rd[a * D] * state->R[b] + Rd[a * D + 1] * state->R[D + b];
			if (D == 3) { m = m + Rd[a * D + 2] * state->R[2 * D + b]; }
			Rn[a * D + b] = m;
		}
	}
	for (int k = 0; k < D * D; ++k) { state->R[k] = Rn[k]; }
	for (int a = 0; a < D; ++a) { state->t[a] = tn[a]; }
	for (int a = 0; a < D; ++a) {
		double s = Rn[a * D] * state->g0[0] + Rn[a * D + 1] * state->g0[1];
		if (D == 3) { s = s + Rn[a * D + 2] * state->g0[2]; }
		state->g[a] = s + tn[a];
	}
	double rot = fabs(delta[0]), tr = fabs(delta[NR]);
	for (int k = 1; k < NR; ++k) { rot = fabs(delta[k]) > rot ? fabs(delta[k]) : rot; }
	for (int k = 1; k < D; ++k) { tr = fabs(delta[NR + k]) > tr ? fabs(delta[NR + k]) : tr; }
	state->last_rotation    = rot;
	state->last_translation = tr;
	state->iterations       = state->iterations + 1;
	state->fixed_mask       = mask;
	if (rot <= rtol && tr <= ttol) {
		state->converged = 1;
		state->stop      = 1;
	}
}

// ---- host side --------------------------------------------------------------------------------------------------------

using namespace prim;  // Arena, arena_alloc, grid
static_assert(kThreads == kGridThreads, "grid() counts work groups of kThreads");

inline int64_t blocks_of(int64_t n) { return (n + kThreads - 1) / kThreads; }

constexpr int kBoundsBlocks = 256;  // the bounds kernel's grid at the most: it strides

// what the two entries share once the target is told apart
struct Target {
	int                 kind = kMesh, D = 0, device = 0;
	const SurfaceIndex* surface = nullptr;
	const fi_mesh*      mesh    = nullptr;  // kMesh: the primitives' vertices (kPlane)
	const NearestIndex* set     = nullptr;
	const float*        normals = nullptr;  // kSet: float[m][D] in `memory`
};

void check_common(long n, const float* source, const fi_register_options* opt, const double* initial, fi_registration* out, int memory,
                  int D)
{
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "the result is null");
	FI_REQUIRE(opt != nullptr, FI_ERR_INVALID, "the options are null");
	FI_REQUIRE(D == 2 || D == 3, FI_ERR_INVALID, "a %d-D target", D);
	FI_REQUIRE(n >= 0, FI_ERR_INVALID, "n = %ld", n);
	FI_REQUIRE(n == 0 || source != nullptr, FI_ERR_INVALID, "source is null");
	FI_REQUIRE(opt->mode == FI_REGISTER_PLANE || opt->mode == FI_REGISTER_POINT, FI_ERR_INVALID, "bad mode %d", opt->mode);
	FI_REQUIRE(opt->max_iterations >= 0, FI_ERR_INVALID, "max_iterations = %d", opt->max_iterations);
	FI_REQUIRE(opt->max_distance >= 0.0f, FI_ERR_INVALID, "max_distance must be >= 0 (got %g)", static_cast<double>(opt->max_distance));  // (NaN fails)
	FI_REQUIRE(opt->rotation_tolerance >= 0.0 && opt->translation_tolerance >= 0.0, FI_ERR_INVALID, "the tolerances must be >= 0 (got %g, %g)",
	           opt->rotation_tolerance, opt->translation_tolerance);
	FI_REQUIRE(opt->loss == FI_LOSS_NONE || opt->loss == FI_LOSS_HUBER || opt->loss == FI_LOSS_CAUCHY || opt->loss == FI_LOSS_TUKEY,
	           FI_ERR_INVALID, "unknown loss %d", opt->loss);
	if (opt->loss != FI_LOSS_NONE) {
		FI_REQUIRE(opt->scale > 0.0f, FI_ERR_INVALID, "a loss needs scale > 0 (got %g)", static_cast<double>(opt->scale));
		FI_REQUIRE(opt->tuning >= 0.0f, FI_ERR_INVALID, "tuning must be >= 0 (got %g)", static_cast<double>(opt->tuning));
	}
	check_memory(memory);
	if (initial) {
		for (int a = 0; a < D; ++a) {
			for (int b = 0; b <= D; ++b) {
				FI_REQUIRE(std::isfinite(initial[a * (D + 1) + b]), FI_ERR_INVALID, "initial[%d][%d] is not finite", a, b);
			}
		}
	}
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld source points in one call", n);
}

template <int D, int MODE>
void launch_pairs_of(int kind, const PairArgs& a, hipStream_t st)
{
	if (kind == kMesh) {
		hipLaunchKernelGGL((k_reg_pairs<D, MODE, kMesh>), grid(a.n), dim3(kThreads), 0, st, a);
	} else {
		hipLaunchKernelGGL((k_reg_pairs<D, MODE, kSet>), grid(a.n), dim3(kThreads), 0, st, a);
	}
}

template <int D>
void launch_pairs(int mode, int kind, const PairArgs& a, hipStream_t st)
{
	if (mode == kPlane) {
		launch_pairs_of<D, kPlane>(kind, a, st);
	} else {
		launch_pairs_of<D, kPoint>(kind, a, st);
	}
	FI_HIP_TRY(hipGetLastError());
}

template <int D>
void run(const Target& tg, int64_t n, const float* source, const fi_register_options* opt, const double* initial, fi_registration* out,
         float* transformed, float* distances, int memory)
{
	Initial start{};
	for (int a = 0; a <= D; ++a) { start.m[a * (D + 1) + a] = 1.0; }
	if (initial) {
		for (int a = 0; a < D; ++a) {
			for (int b = 0; b <= D; ++b) { start.m[a * (D + 1) + b] = initial[a * (D + 1) + b]; }
		}
	}
	if (n == 0) {
		std::memset(out, 0, sizeof(*out));
		for (int k = 0; k < (D + 1) * (D + 1); ++k) { out->transform[k] = start.m[k]; }
		return;
	}
	FI_HIP_TRY(hipSetDevice(tg.device));
	hipStream_t   st    = nullptr;
	const bool    plane = opt->mode == FI_REGISTER_PLANE;
	const int64_t nb    = blocks_of(n), bounds_blocks = std::min<int64_t>(nb, kBoundsBlocks), nw = bounds_blocks * (kThreads / 64);
	const int64_t m     = tg.kind == kSet ? tg.set->n : 0;
	constexpr int K     = sums_of(D);

	const float*     src  = nullptr;
	float *          p = nullptr, *dist = nullptr, *closest = nullptr, *tpos = nullptr, *part = nullptr;
	const float*     tnrm = tg.normals;
	long long*       prim = nullptr;
	double*          partial = nullptr;
	uint64_t*        count   = nullptr;
	RegState*        state   = nullptr;
	fi_registration* res     = nullptr;
	DevBuf           block;
	arena_alloc(block, [&](Arena& ar) {
		state   = ar.take<RegState>(1);
		res     = ar.take<fi_registration>(1);
		part    = ar.take<float>(nw * 2 * D);
		partial = ar.take<double>(nb * K);
		count   = ar.take<uint64_t>(nb);
		prim    = ar.take<long long>(n);
		src     = stage::in(ar, source, n * D, memory, st);
		p       = stage::work(ar, transformed, n * D, memory);
		dist    = stage::work(ar, distances, n, memory);
		if (tg.kind == kMesh) {
			closest = ar.take<float>(n * D);
		} else {
			tpos = ar.take<float>(m * D);
			if (plane) { tnrm = stage::in(ar, tg.normals, m * D, memory, st); }  // (read by the plane mode only)
		}
	});
	if (tg.kind == kSet && tg.set->nf > 0) {
		hipLaunchKernelGGL(k_reg_unsort<D>, grid(tg.set->nf), dim3(kThreads), 0, st, tg.set->nf, m, tg.set->items.as<float4>(), tpos);
	}
	hipLaunchKernelGGL(k_reg_bounds<D>, dim3(static_cast<unsigned>(bounds_blocks)), dim3(kThreads), 0, st, n, src, part);
	hipLaunchKernelGGL(k_reg_init<D>, dim3(1), dim3(64), 0, st, nw, part, start, state);
	FI_HIP_TRY(hipGetLastError());

	PairArgs a{};
	a.n       = n;
	a.p       = p;
	a.dist    = dist;
	a.prim    = prim;
	a.closest = closest;
	a.idx     = tg.mesh ? tg.mesh->idx.as<int>() : nullptr;
	a.pos     = tg.mesh ? tg.mesh->pos.as<float>() : nullptr;
	a.tpos    = tpos;
	a.tnrm    = tnrm;
	a.state   = state;
	a.loss    = opt->loss;
	a.partial = partial;
	a.count   = count;
	if (opt->loss != FI_LOSS_NONE) {
		const float c = opt->tuning > 0.0f ? opt->tuning : (opt->loss == FI_LOSS_HUBER ? 1.345f : opt->loss == FI_LOSS_CAUCHY ? 2.385f : 4.685f);
		a.sc          = static_cast<double>(opt->scale) * static_cast<double>(c);
	}
	// items 2 to 6 of the contract, and the step or the result behind them
	auto evaluate = [&](int final_eval) {
		hipLaunchKernelGGL(k_reg_transform<D>, grid(n), dim3(kThreads), 0, st, n, src, state, p);
		FI_HIP_TRY(hipGetLastError());
		if (tg.kind == kMesh) {
			surface_query(*tg.surface, n, p, opt->max_distance, dist, prim, closest, FI_DEVICE, st);
		} else {
			nearest_query(*tg.set, n, p, opt->max_distance, dist, prim, FI_DEVICE, st);
		}
		launch_pairs<D>(opt->mode, tg.kind, a, st);
		hipLaunchKernelGGL(k_reg_finish<D>, dim3(1), dim3(64), 0, st, n, nb, opt->mode, final_eval, opt->rotation_tolerance,
		                   opt->translation_tolerance, partial, count, state, res);
		FI_HIP_TRY(hipGetLastError());
	};
	for (int it = 0; it < opt->max_iterations; ++it) {
		evaluate(0);
		RegState now;  // (the loop's one read-back a step: whether to go on)
		FI_HIP_TRY(hipMemcpyAsync(&now, state, sizeof(now), hipMemcpyDeviceToHost, st));
		FI_HIP_TRY(hipStreamSynchronize(st));
		if (now.stop) { break; }
	}
	evaluate(1);
	fi_registration got;
	FI_HIP_TRY(hipMemcpyAsync(&got, res, sizeof(got), hipMemcpyDeviceToHost, st));
	stage::back(transformed, p, n * D, memory, st);
	stage::back(distances, dist, n, memory, st);
	FI_HIP_TRY(hipStreamSynchronize(st));  // (the arena goes back behind the kernels that use it)
	*out = got;
}

void dispatch(const Target& tg, long n, const float* source, const fi_register_options* opt, const double* initial, fi_registration* out,
              float* transformed, float* distances, int memory)
{
	if (tg.D == 2) {
		run<2>(tg, n, source, opt, initial, out, transformed, distances, memory);
	} else {
		run<3>(tg, n, source, opt, initial, out, transformed, distances, memory);
	}
}

}  // namespace

void mesh_register(const fi_mesh* target, fi_surface* index, long n, const float* source, const fi_register_options* opt,
                   const double* initial, fi_registration* out, float* transformed, float* distances, int memory)
{
	FI_REQUIRE(target != nullptr || index != nullptr, FI_ERR_INVALID, "null mesh and surface");
	FI_REQUIRE(opt != nullptr, FI_ERR_INVALID, "the options are null");
	FI_REQUIRE(target != nullptr || opt->mode == FI_REGISTER_POINT, FI_ERR_INVALID,
	           "FI_REGISTER_PLANE needs the mesh: a surface alone holds no vertices to take normals from");
	const int D = target ? target->ndim : index->t.D;
	if (target && index) {
		FI_REQUIRE(target->ndim == index->t.D, FI_ERR_INVALID, "a %d-D mesh with a %d-D surface", target->ndim, index->t.D);
		FI_REQUIRE(target->device == index->device, FI_ERR_INVALID, "the mesh is on device %d, the surface on device %d", target->device,
		           index->device);
		FI_REQUIRE(target->np == index->t.np, FI_ERR_INVALID, "the mesh has %lld primitives, the surface %lld",
		           static_cast<long long>(target->np), static_cast<long long>(index->t.np));
	}
	check_common(n, source, opt, initial, out, memory, D);
	Target tg;
	tg.kind   = kMesh;
	tg.D      = D;
	tg.device = target ? target->device : index->device;
	tg.mesh   = target;
	SurfaceIndex own;  // (index null: the structure lives as long as the call)
	if (index) {
		tg.surface = &index->t;
	} else if (n > 0) {
		FI_HIP_TRY(hipSetDevice(target->device));
		surface_build(own, target->ndim, target->nv, target->pos.as<float>(), target->np, target->idx.as<int>(), nullptr);
		tg.surface = &own;
	}
	dispatch(tg, n, source, opt, initial, out, transformed, distances, memory);
}

void points_register(const fi_points* target, const float* target_normals, long n, const float* source, const fi_register_options* opt,
                     const double* initial, fi_registration* out, float* transformed, float* distances, int memory)
{
	FI_REQUIRE(target != nullptr, FI_ERR_INVALID, "null point set");
	FI_REQUIRE(opt != nullptr, FI_ERR_INVALID, "the options are null");
	FI_REQUIRE(target_normals != nullptr || opt->mode != FI_REGISTER_PLANE, FI_ERR_INVALID, "FI_REGISTER_PLANE needs the target's normals");
	check_common(n, source, opt, initial, out, memory, target->t.D);
	Target tg;
	tg.kind    = kSet;
	tg.D       = target->t.D;
	tg.device  = target->device;
	tg.set     = &target->t;
	tg.normals = target_normals;
	dispatch(tg, n, source, opt, initial, out, transformed, distances, memory);
}

}  // namespace fi
