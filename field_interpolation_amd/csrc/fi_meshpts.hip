// fi_meshpts.hip -- points spread over a device mesh by area (2-D: by length), and the distances of such points and of the
// mesh's vertices to another surface reduced to a few figures that are the same bytes on every run.
//
// The contract (include/fi_hip.h fi_mesh_sample / fi_mesh_deviation; tests/meshpts_reference.py is its
// definition in numpy): a primitive's weight is the length of fi_mesh_normals' n_p, scaled by the largest weight into an
// integer of k bits; sample i of n takes the stratum [i, i + 1) / n of the integer weights' total T, a counter-based hash
// (splitmix64's finaliser) places it in the stratum and in the primitive.  fp64 from the fp32 coordinates, one rounding per
// operation (-ffp-contract=off); the prefix sums are integers, hence exact in any order.  Nothing here depends on the run or
// the launch shape.
//
// How it is found:
//   weights    one thread per primitive; a wave's largest weight by shuffles, the waves' maxima by a second kernel of one work
//              group (a maximum does not depend on the order of its reduction).
//   q, C       q_p = floor((w_p / wmax) 2^k) as uint64, scanned exclusively over np + 1 entries (fi_prim.h): entry p + 1 is
//              C_p, entry np the total T -- the call's one read-back, where it must know whether to refuse.
//   samples    k_mpts_sample: hash, stratum, a binary search in the scanned weights from registers, the gather of the
//              primitive's vertices, the point, the normal.  The hot kernel.
//   deviation  the queries (the samples; the used vertices, marked by plain stores of 1, numbered by a scan, compacted) are
//              staged on the device and walked by fi::surface_query, untouched.  k_mpts_reduce sums every block of 256
//              distances by a fixed tree in LDS and takes the block's maximum as an integer key (the distance's bits above,
//              the query's number inverted below: the first of equal maxima wins); one thread adds the block sums in order.
// No floating-point atomics, no atomics at all; one device allocation for every temporary of a call (fi_arena.h).
#include "fi_solver_internal.h"
#include "fi_stage.h"
#include "fi_meshpts.h"
#include "fi_prim.h"
#include "fi_uniform.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace fi {
namespace {

// ---- a primitive ------------------------------------------------------------------------------------------------------

// the vertices of primitive p as doubles, q[corner][axis]
template <int D>
__device__ inline void corners(const int* __restrict__ idx, const float* __restrict__ pos, int64_t p, int64_t v[D], double q[D][D])
{
#pragma unroll
	for (int k = 0; k < D; ++k) {
		v[k] = idx[p * D + k];
#pragma unroll
		for (int d = 0; d < D; ++d) { q[k][d] = static_cast<double>(pos[v[k] * D + d]); }
	}
}

// n_p of fi_mesh_normals (3-D (b - a) x (c - a), 2-D (e_y, -e_x)) and its length, the squares summed in axis order
template <int D>
__device__ inline double face_normal(const double q[D][D], double n[D])
{
	if constexpr (D == 3) {
		double u[3], w[3];
#pragma unroll
		for (int d = 0; d < 3; ++d) {
			u[d] = q[1][d] - q[0][d];
			w[d] = q[2][d] - q[0][d];
		}
		n[0] = u[1] * w[2] - u[2] * w[1];
		n[1] = u[2] * w[0] - u[0] * w[2];
		n[2] = u[0] * w[1] - u[1] * w[0];
		return sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
	} else {
		const double ex = q[1][0] - q[0][0], ey = q[1][1] - q[0][1];
		n[0] = ey;
		n[1] = -ex;
		return sqrt(ex * ex + ey * ey);
	}
}

__device__ inline double wave_max(double x)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) { x = fmax(x, __shfl_xor(x, o, 64)); }
	return x;
}

// ---- weights ----------------------------------------------------------------------------------------------------------

// w[p] (a non-finite one: 0) and the largest of every wave of 64 primitives
template <int D>
__global__ __launch_bounds__(kThreads) void k_mpts_weight(int64_t np, const int* __restrict__ idx, const float* __restrict__ pos,
                                                           double* __restrict__ w, double* __restrict__ wave_top)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	double        x = 0.0;
	if (p < np) {
		int64_t v[D];
		double  q[D][D], n[D];
		corners<D>(idx, pos, p, v, q);
		const double len = face_normal<D>(q, n);
		x                = isfinite(len) ? len : 0.0;
		w[p]             = x;
	}
	x = wave_max(x);
	if ((threadIdx.x & 63) == 0) { wave_top[p >> 6] = x; }
}

// the largest of nw wave maxima, by one work group: its four waves meet in `part` (global memory, written before the barrier
// and read behind it)
__global__ __launch_bounds__(kThreads) void k_mpts_max(int64_t nw, const double* wave_top, double* part, double* wmax)
{
	double x = 0.0;
	for (int64_t j = threadIdx.x; j < nw; j += kThreads) { x = fmax(x, wave_top[j]); }
	x = wave_max(x);
	if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6] = x; }
	__syncthreads();
	if (threadIdx.x == 0) {
		double m = part[0];
		for (int k = 1; k < kThreads / 64; ++k) { m = fmax(m, part[k]); }
		*wmax = m;
	}
}

// q[p] = floor((w[p] / wmax) scale), scale = 2^k; entry np: 0, the place of the scan's total
__global__ __launch_bounds__(kThreads) void k_mpts_q(int64_t np, double scale, const double* __restrict__ w, const double* __restrict__ wmax,
                                                      uint64_t* __restrict__ q)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (p > np) { return; }
	uint64_t     out = 0;
	const double m   = *wmax;
	if (p < np && m > 0.0) {
		double t = w[p] / m;
		t        = t * scale;
		out      = static_cast<uint64_t>(floor(t));
	}
	q[p] = out;
}

// ---- samples ----------------------------------------------------------------------------------------------------------

using counter::uniform;  // fi_uniform.h

struct SampleArgs {
	int64_t         n, np;
	uint64_t        seed, total;  // total: T > 0
	const uint64_t* scanned;      // uint64[np + 1]: entry p + 1 is C_p
	const int*      idx;
	const float*    pos;
	const float*    vnrm;         // the mesh's vertex normals (kVertex)
	float*          out_pos;      // float[n][D]
	float*          out_nrm;      // float[n][D] (kFace, kVertex)
	long long*      out_prim;     // long long[n] or null
};

constexpr int kNoNormals = 0, kFace = 1, kVertex = 2;

template <int D, int NORMALS>
__global__ __launch_bounds__(kThreads) void k_mpts_sample(SampleArgs a)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= a.n) { return; }
	const uint64_t c  = 3 * static_cast<uint64_t>(i);
	const double   xi = uniform(a.seed, c);
	double         r1 = uniform(a.seed, c + 1), r2 = uniform(a.seed, c + 2);
	double         y  = static_cast<double>(i) + xi;
	y                 = y / static_cast<double>(a.n);
	y                 = y * static_cast<double>(a.total);
	uint64_t t        = static_cast<uint64_t>(y);
	if (t >= a.total) { t = a.total - 1; }
	// how many C_p are <= t: t < T = C_(np - 1), so fewer than np
	int64_t lo = 0, hi = a.np;
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (a.scanned[mid + 1] <= t) {
			lo = mid + 1;
		} else {
			hi = mid;
		}
	}
	const int64_t p = lo < a.np ? lo : a.np - 1;
	int64_t       v[D];
	double        q[D][D];
	corners<D>(a.idx, a.pos, p, v, q);
	if constexpr (D == 3) {
		if (r1 + r2 > 1.0) {
			r1 = 1.0 - r1;
			r2 = 1.0 - r2;
		}
	}
#pragma unroll
	for (int d = 0; d < D; ++d) {
		double x = r1 * (q[1][d] - q[0][d]);
		x        = q[0][d] + x;
		if constexpr (D == 3) {
			const double z = r2 * (q[2][d] - q[0][d]);
			x              = x + z;
		}
		a.out_pos[i * D + d] = static_cast<float>(x);
	}
	if (a.out_prim) { a.out_prim[i] = p; }
	if constexpr (NORMALS != kNoNormals) {
		double       f[D];
		const double len = face_normal<D>(q, f);
#pragma unroll
		for (int d = 0; d < D; ++d) { f[d] = f[d] / len; }
		if constexpr (NORMALS == kVertex) {
			double m[D];
			double w0 = 1.0 - r1;
			if constexpr (D == 3) { w0 = w0 - r2; }
#pragma unroll
			for (int d = 0; d < D; ++d) {
				double s = w0 * static_cast<double>(a.vnrm[v[0] * D + d]);
				s        = s + r1 * static_cast<double>(a.vnrm[v[1] * D + d]);
				if constexpr (D == 3) { s = s + r2 * static_cast<double>(a.vnrm[v[2] * D + d]); }
				m[d] = s;
			}
			double l2 = m[0] * m[0] + m[1] * m[1];
			if constexpr (D == 3) { l2 = l2 + m[2] * m[2]; }
			const double ml = sqrt(l2);
			if (ml > 0.0 && isfinite(ml)) {
#pragma unroll
				for (int d = 0; d < D; ++d) { f[d] = m[d] / ml; }
			}
		}
#pragma unroll
		for (int d = 0; d < D; ++d) { a.out_nrm[i * D + d] = static_cast<float>(f[d]); }
	}
}

// ---- the used vertices ------------------------------------------------------------------------------------------------

// (plain stores of the same 1: no atomics)
__global__ __launch_bounds__(kThreads) void k_mpts_mark(int64_t corners, const int* __restrict__ idx, uint32_t* __restrict__ used)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i < corners) { used[idx[i]] = 1; }
}

// the used vertices' positions, in ascending vertex order
template <int D>
__global__ __launch_bounds__(kThreads) void k_mpts_compact(int64_t nv, const uint32_t* __restrict__ used, const uint32_t* __restrict__ number,
                                                            const float* __restrict__ pos, float* __restrict__ out)
{
	const int64_t v = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (v >= nv || !used[v]) { return; }
	const int64_t j = number[v];
#pragma unroll
	for (int d = 0; d < D; ++d) { out[j * D + d] = pos[v * D + d]; }
}

// vertex_distances: a used vertex's distance, NaN for an unused one
__global__ __launch_bounds__(kThreads) void k_mpts_scatter(int64_t nv, const uint32_t* __restrict__ used, const uint32_t* __restrict__ number,
                                                            const float* __restrict__ dist, float* __restrict__ out)
{
	const int64_t v = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (v >= nv) { return; }
	out[v] = used[v] ? dist[number[v]] : NAN;
}

// ---- the reduction ----------------------------------------------------------------------------------------------------

constexpr uint64_t kBeyond = uint64_t(1) << 16, kInvalid = uint64_t(1) << 32;  // a block's three counts (<= 256 each) in one word

// Block b of 256 consecutive queries: S1 and S2 by the tree s[t] += s[t + w], w = 128 .. 1, the tail padded with 0.0; then,
// through the same two arrays, the counts (counted | beyond << 16 | invalid << 32, summed) and the key of the largest
// counted distance (its bits << 32 | ~query: distances are >= 0, so the bits order as the values do; 0: nothing counted).
__global__ __launch_bounds__(kThreads) void k_mpts_reduce(int64_t n, const float* __restrict__ dist, double* __restrict__ s1, double* __restrict__ s2,
                                                           uint64_t* __restrict__ key, uint64_t* __restrict__ count)
{
	__shared__ uint64_t sa[kThreads], sb[kThreads];
	const int     t = threadIdx.x;
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + t;
	double        x = 0.0;
	uint64_t      k = 0, c = 0;
	if (i < n) {
		const float d = dist[i];
		if (isfinite(d)) {
			x = static_cast<double>(d);
			c = 1;
			k = (static_cast<uint64_t>(d > 0.0f ? __float_as_uint(d) : 0u) << 32) | (0xFFFFFFFFu - static_cast<uint32_t>(i));
		} else {
			c = isnan(d) ? kInvalid : kBeyond;
		}
	}
	sa[t] = static_cast<uint64_t>(__double_as_longlong(x));
	sb[t] = static_cast<uint64_t>(__double_as_longlong(x * x));
	__syncthreads();
	for (int w = kThreads / 2; w > 0; w >>= 1) {
		if (t < w) {
			const double u = __longlong_as_double(static_cast<long long>(sa[t])) + __longlong_as_double(static_cast<long long>(sa[t + w]));
			const double v = __longlong_as_double(static_cast<long long>(sb[t])) + __longlong_as_double(static_cast<long long>(sb[t + w]));
			sa[t]          = static_cast<uint64_t>(__double_as_longlong(u));
			sb[t]          = static_cast<uint64_t>(__double_as_longlong(v));
		}
		__syncthreads();
	}
	if (t == 0) {
		s1[blockIdx.x] = __longlong_as_double(static_cast<long long>(sa[0]));
		s2[blockIdx.x] = __longlong_as_double(static_cast<long long>(sb[0]));
	}
	__syncthreads();
	sa[t] = c;
	sb[t] = k;
	__syncthreads();
	for (int w = kThreads / 2; w > 0; w >>= 1) {
		if (t < w) {
			sa[t] = sa[t] + sa[t + w];
			sb[t] = sb[t] > sb[t + w] ? sb[t] : sb[t + w];
		}
		__syncthreads();
	}
	if (t == 0) {
		count[blockIdx.x] = sa[0];
		key[blockIdx.x]   = sb[0];
	}
}

// one thread adds the nb block sums one after the other, ascending, from 0.0, and writes the list's figures
// (launched as one wave: the work is one thread's)
__global__ __launch_bounds__(kThreads) void k_mpts_finish(int64_t n, int64_t nb, int D, const double* __restrict__ s1, const double* __restrict__ s2,
                                                           const uint64_t* __restrict__ key, const uint64_t* __restrict__ count,
                                                           const float* __restrict__ queries, fi_deviation* __restrict__ out)
{
	if (blockIdx.x != 0 || threadIdx.x != 0) { return; }
	double   a = 0.0, b = 0.0;
	uint64_t counted = 0, beyond = 0, invalid = 0, top = 0;
	// (four blocks' partials are loaded before the first of them is added: the additions stay in order, the loads overlap)
	int64_t j = 0;
	for (; j + 4 <= nb; j += 4) {
		const double   a0 = s1[j], a1 = s1[j + 1], a2 = s1[j + 2], a3 = s1[j + 3];
		const double   b0 = s2[j], b1 = s2[j + 1], b2 = s2[j + 2], b3 = s2[j + 3];
		const uint64_t c0 = count[j], c1 = count[j + 1], c2 = count[j + 2], c3 = count[j + 3];
		const uint64_t k0 = key[j], k1 = key[j + 1], k2 = key[j + 2], k3 = key[j + 3];
		a = a + a0;
		a = a + a1;
		a = a + a2;
		a = a + a3;
		b = b + b0;
		b = b + b1;
		b = b + b2;
		b = b + b3;
		const uint64_t c = (c0 + c1) + (c2 + c3);  // (four blocks: each field stays below 2^16)
		counted += c & 0xFFFFu;
		beyond += (c >> 16) & 0xFFFFu;
		invalid += c >> 32;
		const uint64_t k01 = k0 > k1 ? k0 : k1, k23 = k2 > k3 ? k2 : k3, k = k01 > k23 ? k01 : k23;
		top = k > top ? k : top;
	}
	for (; j < nb; ++j) {
		a = a + s1[j];
		b = b + s2[j];
		const uint64_t c = count[j];
		counted += c & 0xFFFFu;
		beyond += (c >> 16) & 0xFFFFu;
		invalid += c >> 32;
		top = key[j] > top ? key[j] : top;
	}
	fi_deviation r;
	r.queries = n;
	r.counted = static_cast<long long>(counted);
	r.beyond  = static_cast<long long>(beyond);
	r.invalid = static_cast<long long>(invalid);
	r.at      = -1;
	r.max = r.mean = r.rms = 0.0;
	r.where[0] = r.where[1] = r.where[2] = 0.0f;
	if (counted > 0) {
		const double m = static_cast<double>(counted);
		r.at           = static_cast<long long>(0xFFFFFFFFu - static_cast<uint32_t>(top & 0xFFFFFFFFu));
		r.max          = static_cast<double>(__uint_as_float(static_cast<uint32_t>(top >> 32)));
		r.mean         = a / m;
		r.rms          = sqrt(b / m);
		// (constant indices: an array indexed by a loop variable would be moved into LDS)
		r.where[0] = queries[r.at * D];
		r.where[1] = queries[r.at * D + 1];
		if (D == 3) { r.where[2] = queries[r.at * D + 2]; }
	}
	*out = r;
}

// ---- host side --------------------------------------------------------------------------------------------------------

using namespace prim;  // Arena, Scratch, scan_u32, scan_u64, read_u32, bits_for, grid
static_assert(kThreads == kGridThreads, "grid() counts work groups of kThreads");

inline int64_t blocks_of(int64_t n) { return (n + kThreads - 1) / kThreads; }

// the temporaries of the sampler's passes before its hot kernel
struct Weights {
	double *  w, *wave_top, *part, *wmax;
	uint64_t *q, *scanned;
	int64_t   waves;
};

void take_weights(Arena& a, int64_t np, Weights& w)
{
	w.waves    = blocks_of(np > 0 ? np : 1) * (kThreads / 64);
	w.w        = a.take<double>(np);
	w.wave_top = a.take<double>(w.waves);
	w.part     = a.take<double>(kThreads / 64);
	w.wmax     = a.take<double>(1);
	w.q        = a.take<uint64_t>(np + 1);
	w.scanned  = a.take<uint64_t>(np + 1);
}

// passes 1 to 3 and the read-back: T (m has primitives)
template <int D>
uint64_t scan_weights_of(const fi_mesh* m, const Weights& w, const Scratch& tmp, hipStream_t st)
{
	const int64_t np = m->np;
	const int     k  = std::min(32, 52 - bits_for(np));
	hipLaunchKernelGGL(k_mpts_weight<D>, grid(np), dim3(kThreads), 0, st, np, m->idx.as<int>(), m->pos.as<float>(), w.w, w.wave_top);
	hipLaunchKernelGGL(k_mpts_max, dim3(1), dim3(kThreads), 0, st, w.waves, w.wave_top, w.part, w.wmax);
	hipLaunchKernelGGL(k_mpts_q, grid(np + 1), dim3(kThreads), 0, st, np, std::ldexp(1.0, k), w.w, w.wmax, w.q);
	FI_HIP_TRY(hipGetLastError());
	scan_u64(w.q, w.scanned, np + 1, tmp, st);
	uint64_t total = 0;
	FI_HIP_TRY(hipMemcpyAsync(&total, w.scanned + np, sizeof(total), hipMemcpyDeviceToHost, st));
	FI_HIP_TRY(hipStreamSynchronize(st));
	return total;
}

template <int D>
void launch_sample(int mode, const SampleArgs& a, hipStream_t st)
{
	if (mode == kNoNormals) {
		hipLaunchKernelGGL((k_mpts_sample<D, kNoNormals>), grid(a.n), dim3(kThreads), 0, st, a);
	} else if (mode == kFace) {
		hipLaunchKernelGGL((k_mpts_sample<D, kFace>), grid(a.n), dim3(kThreads), 0, st, a);
	} else {
		hipLaunchKernelGGL((k_mpts_sample<D, kVertex>), grid(a.n), dim3(kThreads), 0, st, a);
	}
	FI_HIP_TRY(hipGetLastError());
}

// n samples of m (T = total > 0) into device arrays
void draw(const fi_mesh* m, int64_t n, uint64_t seed, int mode, uint64_t total, const Weights& w, float* positions, float* normals,
          long long* primitives, hipStream_t st)
{
	SampleArgs a{};
	a.n        = n;
	a.np       = m->np;
	a.seed     = seed;
	a.total    = total;
	a.scanned  = w.scanned;
	a.idx      = m->idx.as<int>();
	a.pos      = m->pos.as<float>();
	a.vnrm     = m->has_normals ? m->nrm.as<float>() : nullptr;
	a.out_pos  = positions;
	a.out_nrm  = normals;
	a.out_prim = primitives;
	if (m->ndim == 2) {
		launch_sample<2>(mode, a, st);
	} else {
		launch_sample<3>(mode, a, st);
	}
}

uint64_t scan_weights(const fi_mesh* m, const Weights& w, const Scratch& tmp, hipStream_t st)
{
	return m->ndim == 2 ? scan_weights_of<2>(m, w, tmp, st) : scan_weights_of<3>(m, w, tmp, st);
}

// the partial results of a reduction over at most `blocks` blocks
struct Partials {
	double *  s1, *s2;
	uint64_t *key, *count;
};

void take_partials(Arena& a, int64_t blocks, Partials& p)
{
	p.s1    = a.take<double>(blocks);
	p.s2    = a.take<double>(blocks);
	p.key   = a.take<uint64_t>(blocks);
	p.count = a.take<uint64_t>(blocks);
}

// the figures of n > 0 distances (queries: their positions), into *out on the device
void reduce(int64_t n, int D, const float* dist, const float* queries, const Partials& p, fi_deviation* out, hipStream_t st)
{
	const int64_t nb = blocks_of(n);
	hipLaunchKernelGGL(k_mpts_reduce, grid(n), dim3(kThreads), 0, st, n, dist, p.s1, p.s2, p.key, p.count);
	hipLaunchKernelGGL(k_mpts_finish, dim3(1), dim3(64), 0, st, n, nb, D, p.s1, p.s2, p.key, p.count, queries, out);
	FI_HIP_TRY(hipGetLastError());
}

fi_deviation nothing()
{
	fi_deviation r;
	std::memset(&r, 0, sizeof(r));
	r.at = -1;
	return r;
}

}  // namespace

void mesh_sample(const fi_mesh* m, long n, unsigned long long seed, int normals_mode, float* positions, float* normals, long long* primitives,
                 int memory)
{
	FI_REQUIRE(m != nullptr, FI_ERR_INVALID, "null mesh");
	FI_REQUIRE(n >= 0, FI_ERR_INVALID, "n = %ld", n);
	FI_REQUIRE(n == 0 || positions != nullptr, FI_ERR_INVALID, "positions is null");
	FI_REQUIRE(normals_mode == FI_SAMPLE_NORMALS_FACE || normals_mode == FI_SAMPLE_NORMALS_VERTEX, FI_ERR_INVALID, "bad normals mode %d",
	           normals_mode);
	check_memory(memory);
	FI_REQUIRE(!(normals && normals_mode == FI_SAMPLE_NORMALS_VERTEX) || m->has_normals, FI_ERR_INVALID, "the mesh has no vertex normals");
	FI_REQUIRE(m->ndim == 2 || m->ndim == 3, FI_ERR_INVALID, "a mesh of %d-vertex primitives", m->ndim);
	// (one thread per sample, (double)i exact)
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld samples in one call", n);
	if (n == 0) { return; }
	FI_REQUIRE(m->np > 0, FI_ERR_INVALID, "the mesh has no primitives to sample");
	FI_HIP_TRY(hipSetDevice(m->device));
	hipStream_t   st   = nullptr;
	const int64_t D    = m->ndim;
	Weights       w{};
	Scratch       tmp{};
	float *       dpos = nullptr, *dnrm = nullptr;
	long long*    dprim = nullptr;
	const size_t  tmp_bytes = scan_u64_bytes(m->np + 1);
	DevBuf        block;
	arena_alloc(block, [&](Arena& a) {
		take_weights(a, m->np, w);
		dpos      = stage::out(a, positions, n * D, memory);
		dnrm      = stage::out(a, normals, n * D, memory);
		dprim     = stage::out(a, primitives, n, memory);
		tmp.p     = a.take<char>(static_cast<int64_t>(tmp_bytes));
		tmp.bytes = tmp_bytes;
	});
	const uint64_t total = scan_weights(m, w, tmp, st);  // (the call's one synchronisation before its outputs)
	FI_REQUIRE(total > 0, FI_ERR_INVALID, "no primitive of the mesh has a positive finite measure");
	const int mode = !normals ? kNoNormals : normals_mode == FI_SAMPLE_NORMALS_FACE ? kFace : kVertex;
	draw(m, n, seed, mode, total, w, dpos, dnrm, dprim, st);
	stage::back(positions, dpos, n * D, memory, st);
	stage::back(normals, dnrm, n * D, memory, st);
	stage::back(primitives, dprim, n, memory, st);
	FI_HIP_TRY(hipStreamSynchronize(st));  // (the arena goes back behind the kernels that use it)
}

void mesh_deviation(const fi_mesh* a, fi_surface* b, long samples, unsigned long long seed, float max_distance, fi_deviation* of_samples,
                    fi_deviation* of_vertices, float* vertex_distances, int memory)
{
	FI_REQUIRE(a != nullptr && b != nullptr, FI_ERR_INVALID, "null mesh or surface");
	FI_REQUIRE(of_samples || of_vertices || vertex_distances, FI_ERR_INVALID, "nothing is asked for");
	FI_REQUIRE(a->ndim == 2 || a->ndim == 3, FI_ERR_INVALID, "a mesh of %d-vertex primitives", a->ndim);
	FI_REQUIRE(a->ndim == b->t.D, FI_ERR_INVALID, "a %d-D mesh against a %d-D surface", a->ndim, b->t.D);
	FI_REQUIRE(a->device == b->device, FI_ERR_INVALID, "the mesh is on device %d, the surface on device %d", a->device, b->device);
	FI_REQUIRE(samples >= 0, FI_ERR_INVALID, "samples = %ld", samples);
	FI_REQUIRE(max_distance >= 0.0f, FI_ERR_INVALID, "max_distance must be >= 0 (got %g)", static_cast<double>(max_distance));  // (NaN fails)
	check_memory(memory);
	FI_REQUIRE(samples < (1L << 31), FI_ERR_UNSUPPORTED, "%ld samples in one call", samples);
	FI_HIP_TRY(hipSetDevice(a->device));
	hipStream_t   st = nullptr;
	const int     D  = a->ndim;
	const int64_t nv = a->nv, np = a->np, ns = samples;
	const bool    sampled = ns > 0 && of_samples && np > 0;
	const bool    walked  = (of_vertices || vertex_distances) && nv > 0;

	Weights       w{};
	Partials      p{};
	Scratch       tmp{};
	float *       spos = nullptr, *sdist = nullptr, *vpos = nullptr, *vdist = nullptr, *vout = vertex_distances;
	uint32_t *    used = nullptr, *number = nullptr;
	fi_deviation* res  = nullptr;
	size_t        tmp_bytes = 0;
	if (sampled) { tmp_bytes = scan_u64_bytes(np + 1); }
	if (walked) { tmp_bytes = std::max(tmp_bytes, scan_bytes(nv + 1)); }
	DevBuf block;
	arena_alloc(block, [&](Arena& ar) {
		res = ar.take<fi_deviation>(2);
		take_partials(ar, std::max(blocks_of(ns), blocks_of(nv)), p);
		if (sampled) {
			take_weights(ar, np, w);
			spos  = ar.take<float>(ns * D);
			sdist = ar.take<float>(ns);
		}
		if (walked) {
			used   = ar.take<uint32_t>(nv + 1);
			number = ar.take<uint32_t>(nv + 1);
			vpos   = ar.take<float>(nv * D);
			vdist  = ar.take<float>(nv);
			vout   = stage::out(ar, vertex_distances, nv, memory);
		}
		tmp.p     = ar.take<char>(static_cast<int64_t>(tmp_bytes));
		tmp.bytes = tmp_bytes;
	});

	fi_deviation host[2] = {nothing(), nothing()};
	bool         have[2] = {false, false};
	if (sampled) {
		const uint64_t total = scan_weights(a, w, tmp, st);
		if (total > 0) {
			draw(a, ns, seed, kNoNormals, total, w, spos, nullptr, nullptr, st);
			surface_query(b->t, ns, spos, max_distance, sdist, nullptr, nullptr, FI_DEVICE, st);
			reduce(ns, D, sdist, spos, p, res, st);
			have[0] = true;
		}
	}
	if (walked) {
		FI_HIP_TRY(hipMemsetAsync(used, 0, sizeof(uint32_t) * (nv + 1), st));
		if (np > 0) { hipLaunchKernelGGL(k_mpts_mark, grid(np * D), dim3(kThreads), 0, st, np * D, a->idx.as<int>(), used); }
		FI_HIP_TRY(hipGetLastError());
		scan_u32(used, number, nv + 1, tmp, st);
		const int64_t count = read_u32(number + nv, st);
		if (count > 0) {
			if (D == 2) {
				hipLaunchKernelGGL(k_mpts_compact<2>, grid(nv), dim3(kThreads), 0, st, nv, used, number, a->pos.as<float>(), vpos);
			} else {
				hipLaunchKernelGGL(k_mpts_compact<3>, grid(nv), dim3(kThreads), 0, st, nv, used, number, a->pos.as<float>(), vpos);
			}
			FI_HIP_TRY(hipGetLastError());
			surface_query(b->t, count, vpos, max_distance, vdist, nullptr, nullptr, FI_DEVICE, st);
			if (of_vertices) {
				reduce(count, D, vdist, vpos, p, res + 1, st);  // (behind the samples' on the same stream: the partials are free again)
				have[1] = true;
			}
		}
		if (vertex_distances) {
			hipLaunchKernelGGL(k_mpts_scatter, grid(nv), dim3(kThreads), 0, st, nv, used, number, vdist, vout);
			FI_HIP_TRY(hipGetLastError());
			stage::back(vertex_distances, vout, nv, memory, st);
		}
	}
	for (int k = 0; k < 2; ++k) {
		if (have[k]) { FI_HIP_TRY(hipMemcpyAsync(&host[k], res + k, sizeof(fi_deviation), hipMemcpyDeviceToHost, st)); }
	}
	FI_HIP_TRY(hipStreamSynchronize(st));
	if (of_samples) { *of_samples = host[0]; }
	if (of_vertices) { *of_vertices = host[1]; }
}

}  // namespace fi
