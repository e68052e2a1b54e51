// fi_dual.hip -- dual contouring of a lattice field (2-D: segments, 3-D: triangles), on the device.
//
// The contract (include/fi_hip.h fi_dual_contour): d = f - iso in fp32, inside is d <= 0; one vertex per cell
// whose corners are not all on one side, placed by the reference's regularised least-squares fit (src/dual_contouring_2d.cpp)
// to the planes of the corner gradients, keyed by the linear index of the cell's lowest corner; one primitive per crossing
// lattice edge whose surrounding cells all exist, emitted by the lowest of them.  Passes:
//   k_dc_count     one thread per cell: is it active, how many primitives it emits; summed per workgroup; the non-finite flag
//   (scan)         exclusive sums of the workgroup totals (rocPRIM); the two grand totals and the flag read back once
//   k_dc_compact   one thread per cell again: the active cells' keys at their scanned slots and their first primitive
//   k_dc_emit      one thread per ACTIVE cell: the vertex fit, position and normal, then its primitives, the neighbouring
//                  cells' vertex numbers found by a galloping search in the ascending keys
// Only the first two read the whole field; the fit and the primitives touch the active cells and their neighbourhoods.
// Scratch: 8 bytes per active cell (the first primitives) plus the workgroup totals; nothing per lattice point.
#include "fi_solver_internal.h"
#include "fi_stage.h"
#include "fi_prim.h"
#include "fi_dual.h"

namespace fi {

namespace {

constexpr int kDualThreads = 256;
constexpr int kMaxSolves   = 32;

struct DualView {
	const float* f;      // the field, x fastest
	const float* g;      // the caller's gradients (D per point, interleaved) or nullptr: central differences of d
	int     n[3];        // extents (1 beyond ndim)
	int     cn[3];       // cells per axis, n - 1 (1 beyond ndim)
	float   iso;
	int64_t ncell;
};

__device__ inline float dval(const DualView& v, int64_t i) { return v.f[i] - v.iso; }

// the lattice index of the point at c
__device__ inline int64_t lin(const DualView& v, const int* c)
{
	return c[0] + static_cast<int64_t>(v.n[0]) * (c[1] + static_cast<int64_t>(v.n[1]) * c[2]);
}

// lowest corner of dense cell number i (x fastest over the cells)
template <int D>
__device__ inline void cell_of(const DualView& v, int64_t i, int* c)
{
	const int64_t r = i / v.cn[0];
	c[0] = static_cast<int>(i - r * v.cn[0]);
	if (D == 2) {
		c[1] = static_cast<int>(r);
		c[2] = 0;
	} else {
		const int64_t s = r / v.cn[1];
		c[1] = static_cast<int>(r - s * v.cn[1]);
		c[2] = static_cast<int>(s);
	}
}

// corner k of the cell whose lowest corner is `base` (bit a of k: +1 along axis a)
template <int D>
__device__ inline int64_t corner(const DualView& v, int64_t base, int k)
{
	const int64_t s1 = v.n[0], s2 = static_cast<int64_t>(v.n[0]) * v.n[1];
	return base + (k & 1) + ((k >> 1) & 1) * s1 + (D == 3 ? ((k >> 2) & 1) * s2 : 0);
}

// bit k: corner k is inside (d <= 0); *bad: a non-finite d among them
template <int D>
__device__ inline unsigned inside_mask(const DualView& v, int64_t base, float* d, bool* bad)
{
	unsigned m = 0;
#pragma unroll
	for (int k = 0; k < (1 << D); ++k) {
		d[k] = dval(v, corner<D>(v, base, k));
		*bad = *bad || !isfinite(d[k]);
		if (d[k] <= 0.0f) { m |= 1u << k; }
	}
	return m;
}

__device__ inline bool active(unsigned m, int D) { return m != 0 && m != (1u << (1 << D)) - 1; }

// bit a: the cell emits the primitive of the lattice edge (p, p + e_a), p = c + sum_(k != a) e_k -- its ends differ in
// inside-ness and every cell around it exists (c_k <= n_k - 3 for k != a)
template <int D>
__device__ inline unsigned emits(const DualView& v, const int* c, unsigned m)
{
	constexpr int top = (1 << D) - 1;
	unsigned out = 0;
#pragma unroll
	for (int a = 0; a < D; ++a) {
		bool ok = true;
#pragma unroll
		for (int k = 0; k < D; ++k) { ok = ok && (k == a || c[k] + 3 <= v.n[k]); }
		const int near = top ^ (1 << a);
		if (ok && (((m >> near) ^ (m >> top)) & 1u)) { out |= 1u << a; }
	}
	return out;
}

// (is the cell active, its primitives) of dense cell i; *base: its lowest corner's lattice index
template <int D>
__device__ inline void cell_counts(const DualView& v, int64_t i, int64_t* base, uint32_t* nv, uint32_t* np, bool* bad)
{
	int c[3];
	cell_of<D>(v, i, c);
	*base = lin(v, c);
	float d[1 << D];
	const unsigned m = inside_mask<D>(v, *base, d, bad);
	*nv = active(m, D) ? 1u : 0u;
	*np = static_cast<uint32_t>(__popc(emits<D>(v, c, m))) * (D == 2 ? 1u : 2u);
}

template <int D>
__global__ __launch_bounds__(kDualThreads) void k_dc_count(DualView v, uint32_t* __restrict__ wg_v, uint32_t* __restrict__ wg_p,
                                                           uint32_t* __restrict__ flag)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kDualThreads + threadIdx.x;
	uint32_t nv = 0, np = 0;
	bool bad = false;
	if (i < v.ncell) {
		int64_t base = 0;
		cell_counts<D>(v, i, &base, &nv, &np, &bad);
	}
	if (__any(bad) && (threadIdx.x & 63) == 0) { atomicOr(flag, 1u); }
	uint32_t tv = 0, tp = 0;
	(void)block_scan<kDualThreads>(nv, &tv);
	__syncthreads();
	(void)block_scan<kDualThreads>(np, &tp);
	if (threadIdx.x == 0) {
		wg_v[blockIdx.x] = tv;
		wg_p[blockIdx.x] = tp;
	}
}

__global__ void k_dc_totals(const uint64_t* __restrict__ sv, const uint64_t* __restrict__ sp, const uint32_t* __restrict__ flag,
                            int64_t nb, uint64_t* __restrict__ out)
{
	out[0] = sv[nb];
	out[1] = sp[nb];
	out[2] = *flag;
}

template <int D>
__global__ __launch_bounds__(kDualThreads) void k_dc_compact(DualView v, const uint64_t* __restrict__ off_v,
                                                             const uint64_t* __restrict__ off_p, int64_t* __restrict__ key,
                                                             uint64_t* __restrict__ first_prim)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kDualThreads + threadIdx.x;
	uint32_t nv = 0, np = 0;
	int64_t base = 0;
	bool bad = false;
	if (i < v.ncell) { cell_counts<D>(v, i, &base, &nv, &np, &bad); }
	uint32_t tv = 0, tp = 0;
	const uint32_t pv = block_scan<kDualThreads>(nv, &tv);
	__syncthreads();
	const uint32_t pp = block_scan<kDualThreads>(np, &tp);
	if (nv == 0) { return; }
	const uint64_t k = off_v[blockIdx.x] + pv;
	key[k] = base;
	first_prim[k] = off_p[blockIdx.x] + pp;
}

// the gradient component along axis a at point p (coordinates q, d = dp): the caller's, or the reference's
// calculate_gradients -- one-sided at that axis's own border, (d[+1] - d[-1]) / 2 inside
template <int D>
__device__ inline float grad(const DualView& v, int64_t p, const int* q, int a, float dp)
{
	if (v.g) { return v.g[p * D + a]; }
	const int64_t s = a == 0 ? 1 : (a == 1 ? static_cast<int64_t>(v.n[0]) : static_cast<int64_t>(v.n[0]) * v.n[1]);
	if (q[a] == 0) { return dval(v, p + s) - dp; }
	if (q[a] == v.n[a] - 1) { return dp - dval(v, p - s); }
	return (dval(v, p + s) - dval(v, p - s)) * 0.5f;
}

// the index of key t among key[j + 1 .. nv - 1] (ascending, key[j] < t, t present): gallop, then bisect
__device__ inline int find_after(const int64_t* __restrict__ key, int64_t nv, int64_t j, int64_t t)
{
	int64_t lo = j, step = 1;  // key[lo] < t
	while (lo + step < nv && key[lo + step] < t) {
		lo += step;
		step <<= 1;
	}
	int64_t hi = lo + step < nv ? lo + step : nv - 1;  // key[hi] >= t
	while (hi - lo > 1) {
		const int64_t mid = lo + ((hi - lo) >> 1);
		if (key[mid] < t) {
			lo = mid;
		} else {
			hi = mid;
		}
	}
	return static_cast<int>(hi);
}

// 2-D: the reference's solve_lin_eq_2d; 3-D: Cramer's rule, each determinant by its first-row cofactor expansion
__device__ inline float det3(float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7, float a8)
{
	const float c0 = a4 * a8 - a5 * a7;
	const float c1 = a3 * a8 - a5 * a6;
	const float c2 = a3 * a7 - a4 * a6;
	return (a0 * c0 - a1 * c1) + a2 * c2;
}

template <int D>
__device__ inline void solve(const float* M, const float* b, float* x)
{
	if (D == 2) {
		const float det = M[0] * M[3] - M[1] * M[2];
		x[0] = (b[0] * M[3] - M[1] * b[1]) / det;
		x[1] = (b[1] * M[0] - M[2] * b[0]) / det;
	} else {
		const float det = det3(M[0], M[1], M[2], M[3], M[4], M[5], M[6], M[7], M[8]);
		x[0] = det3(b[0], M[1], M[2], b[1], M[4], M[5], b[2], M[7], M[8]) / det;
		x[1] = det3(M[0], b[0], M[2], M[3], b[1], M[5], M[6], b[2], M[8]) / det;
		x[2] = det3(M[0], M[1], b[0], M[3], M[4], b[1], M[6], M[7], b[2]) / det;
	}
}

template <int D>
__global__ __launch_bounds__(kDualThreads) void k_dc_emit(DualView v, int64_t nv, const int64_t* __restrict__ key,
                                                          const uint64_t* __restrict__ first_prim, float* __restrict__ pos,
                                                          float* __restrict__ nrm, int* __restrict__ idx)
{
	constexpr int NC = 1 << D;
	const int64_t j = static_cast<int64_t>(blockIdx.x) * kDualThreads + threadIdx.x;
	if (j >= nv) { return; }
	const int64_t base = key[j];
	int c[3];
	{
		const int64_t r = base / v.n[0];
		c[0] = static_cast<int>(base - r * v.n[0]);
		const int64_t s = r / v.n[1];
		c[1] = static_cast<int>(r - s * v.n[1]);
		c[2] = static_cast<int>(s);
	}
	float d[NC];
	bool bad = false;
	const unsigned m = inside_mask<D>(v, base, d, &bad);
	float g[NC][D];
#pragma unroll
	for (int k = 0; k < NC; ++k) {
		const int q[3] = {c[0] + (k & 1), c[1] + ((k >> 1) & 1), c[2] + (D == 3 ? (k >> 2) & 1 : 0)};
		const int64_t p = corner<D>(v, base, k);
#pragma unroll
		for (int a = 0; a < D; ++a) { g[k][a] = grad<D>(v, p, q, a, d[k]); }
	}

	// A^T A and A^T b over the corner rows: A_k = g_k, b_k = ((bit_0 g_0 + bit_1 g_1) + bit_2 g_2) - d_k, a zero row where no
	// cell edge at corner k crosses
	float M[D * D], r[D];
#pragma unroll
	for (int e = 0; e < D * D; ++e) { M[e] = 0.0f; }
#pragma unroll
	for (int e = 0; e < D; ++e) { r[e] = 0.0f; }
#pragma unroll
	for (int k = 0; k < NC; ++k) {
		bool cross = false;
#pragma unroll
		for (int a = 0; a < D; ++a) { cross = cross || (((m >> k) ^ (m >> (k ^ (1 << a)))) & 1u); }
		float A[D];
#pragma unroll
		for (int a = 0; a < D; ++a) { A[a] = cross ? g[k][a] : 0.0f; }
		float s = static_cast<float>(k & 1) * A[0] + static_cast<float>((k >> 1) & 1) * A[1];
		if (D == 3) { s = s + static_cast<float>((k >> 2) & 1) * A[D - 1]; }
		const float b = cross ? s - d[k] : 0.0f;
#pragma unroll
		for (int a = 0; a < D; ++a) {
#pragma unroll
			for (int e = 0; e < D; ++e) { M[D * a + e] = M[D * a + e] + A[a] * A[e]; }
			r[a] = r[a] + A[a] * b;
		}
	}
	// the regularisation rows reg e_k (right-hand side 0.5 reg), reg doubling from 0.001 while the vertex leaves the unit cell
	// (a NaN ends the loop, as the reference's do ... while); at most kMaxSolves solves
	float x[D];
	float reg = 0.001f;
	for (int it = 0; it < kMaxSolves; ++it) {
		float Mi[D * D], ri[D];
#pragma unroll
		for (int e = 0; e < D * D; ++e) { Mi[e] = M[e]; }
#pragma unroll
		for (int e = 0; e < D; ++e) { ri[e] = r[e]; }
		const float br = 0.5f * reg;
#pragma unroll
		for (int row = 0; row < D; ++row) {
			float A[D];
#pragma unroll
			for (int a = 0; a < D; ++a) { A[a] = a == row ? reg : 0.0f; }
#pragma unroll
			for (int a = 0; a < D; ++a) {
#pragma unroll
				for (int e = 0; e < D; ++e) { Mi[D * a + e] = Mi[D * a + e] + A[a] * A[e]; }
				ri[a] = ri[a] + A[a] * br;
			}
		}
		solve<D>(Mi, ri, x);
		reg = reg * 2.0f;
		bool out = false;
#pragma unroll
		for (int a = 0; a < D; ++a) { out = out || x[a] < 0.0f || x[a] > 1.0f; }
		if (!out) { break; }
	}
	bool ok = true;
#pragma unroll
	for (int a = 0; a < D; ++a) { ok = ok && x[a] >= 0.0f && x[a] <= 1.0f; }  // (NaN fails)
#pragma unroll
	for (int a = 0; a < D; ++a) {
		if (!ok) { x[a] = 0.5f; }
		pos[j * D + a] = static_cast<float>(c[a]) + x[a];
	}

	// the normal: the corner gradients under fi_sample's linear weights at the in-cell offset, normalised
	float u[D][2];
#pragma unroll
	for (int a = 0; a < D; ++a) {
		u[a][0] = 1.0f - x[a];
		u[a][1] = x[a];
	}
	float nv3[D], len2 = 0.0f;
#pragma unroll
	for (int a = 0; a < D; ++a) {
		float acc = 0.0f;
#pragma unroll
		for (int k = 0; k < NC; ++k) {
			float w = u[0][k & 1];
#pragma unroll
			for (int e = 1; e < D; ++e) { w = w * u[e][(k >> e) & 1]; }
			const float term = w * g[k][a];
			acc = k == 0 ? term : acc + term;
		}
		nv3[a] = acc;
		len2 = len2 + acc * acc;
	}
	const float len = sqrtf(len2);
#pragma unroll
	for (int a = 0; a < D; ++a) { nrm[j * D + a] = len > 0.0f ? nv3[a] / len : 0.0f; }

	// the primitives, axis a from D - 1 down to 0
	const unsigned em = emits<D>(v, c, m);
	if (em == 0) { return; }
	const int64_t st[3] = {1, v.n[0], static_cast<int64_t>(v.n[0]) * v.n[1]};
	const int me = static_cast<int>(j);
	uint64_t o = first_prim[j];
	constexpr int top = NC - 1;
	if (D == 2) {
		const bool far = (m >> top) & 1u;
		if (em & 2u) {  // the +x neighbour: (this, it) when the far end is inside
			const int nb = find_after(key, nv, j, base + 1);
			idx[2 * o]     = far ? me : nb;
			idx[2 * o + 1] = far ? nb : me;
			++o;
		}
		if (em & 1u) {  // the +y neighbour: (it, this) when the far end is inside
			const int nb = find_after(key, nv, j, base + st[1]);
			idx[2 * o]     = far ? nb : me;
			idx[2 * o + 1] = far ? me : nb;
		}
	} else {
#pragma unroll
		for (int a = D - 1; a >= 0; --a) {
			if (!((em >> a) & 1u)) { continue; }
			const int64_t sb = st[(a + 1) % 3], sc = st[(a + 2) % 3];
			const int q1 = find_after(key, nv, j, base + sb);
			const int q2 = find_after(key, nv, j, base + sb + sc);
			const int q3 = find_after(key, nv, j, base + sc);
			const bool keep = (m >> (top ^ (1 << a))) & 1u;  // the near end is inside: the quad's normal +a points outwards
			int* t = idx + 3 * o;
			t[0] = me;
			t[1] = keep ? q1 : q3;
			t[2] = q2;
			t[3] = me;
			t[4] = q2;
			t[5] = keep ? q3 : q1;
			o += 2;
		}
	}
}

template <int D>
void run(const DualView& v0, hipStream_t st, fi_mesh* m)
{
	DualView v = v0;
	m->ndim = D;
	m->nv = m->np = 0;
	v.ncell = 1;
	for (int a = 0; a < D; ++a) {
		if (v.n[a] < 2) { return; }
		v.ncell *= v.cn[a];
	}
	const int64_t nb = (v.ncell + kDualThreads - 1) / kDualThreads;
	const dim3    groups(static_cast<unsigned>(nb)), threads(kDualThreads);
	ExtractScans  s;
	const bool    any = extract_sizes<D>(
		nb, st, m, s,
		[&](uint32_t* wg_v, uint32_t* wg_p, uint32_t* flag) { hipLaunchKernelGGL((k_dc_count<D>), groups, threads, 0, st, v, wg_v, wg_p, flag); },
		[&](const uint64_t* sv, const uint64_t* sp, const uint32_t* flag, uint64_t* tot) {
			hipLaunchKernelGGL(k_dc_totals, dim3(1), dim3(1), 0, st, sv, sp, flag, nb, tot);
		});
	if (!any) { return; }
	DevBuf first;
	first.alloc(sizeof(uint64_t) * m->nv);
	hipLaunchKernelGGL((k_dc_compact<D>), groups, threads, 0, st, v, s.sv, s.sp, m->key.as<int64_t>(), first.as<uint64_t>());
	FI_HIP_TRY(hipGetLastError());
	const int64_t ne = (m->nv + kDualThreads - 1) / kDualThreads;
	hipLaunchKernelGGL((k_dc_emit<D>), dim3(static_cast<unsigned>(ne)), threads, 0, st, v, m->nv, m->key.as<int64_t>(), first.as<uint64_t>(),
	                   m->pos.as<float>(), m->nrm.as<float>(), m->idx.as<int>());
	FI_HIP_TRY(hipGetLastError());
	FI_HIP_TRY(hipStreamSynchronize(st));
}

void check_dims(int ndim, const int* sizes) { check_mesh_dims(ndim, sizes, "dual contouring of a 1-D lattice is not supported"); }

}  // namespace

void dual_contour_whole(const float* field, const float* gradients, int ndim, const int* sizes, float iso, hipStream_t st,
                        fi_mesh** out)
{
	check_dims(ndim, sizes);
	DualView v{};
	v.f   = field;
	v.g   = gradients;
	v.iso = iso;
	for (int d = 0; d < 3; ++d) {
		v.n[d]  = d < ndim ? sizes[d] : 1;
		v.cn[d] = d < ndim ? sizes[d] - 1 : 1;
	}
	std::unique_ptr<fi_mesh> m(new fi_mesh());
	FI_HIP_TRY(hipGetDevice(&m->device));
	if (ndim == 2) {
		run<2>(v, st, m.get());
	} else {
		run<3>(v, st, m.get());
	}
	*out = m.release();
}

void dual_contour_ctx(fi_ctx* c, const float* field, const float* gradients, float iso, int memory, fi_mesh** out)
{
	const Geom& g = c->g;
	check_dims(g.ndim, g.gn);
	FI_REQUIRE(c->nranks == 1, FI_ERR_UNSUPPORTED,
	           "dual contouring of a slab context: a slab's vertices need field planes hi .. hi + 2, one more than the ghost "
	           "planes the iso path exchanges (a vertex exchange is not implemented)");
	FI_REQUIRE(field || c->vectors_ready, FI_ERR_STATE, "no solution yet");
	if (field || gradients) { check_memory(memory); }
	AllocStream alloc_on(c->stream);
	DevBuf buf;
	const float* f = field_f32(c, field, memory, buf);
	stage::In<float> gr(gradients, static_cast<int64_t>(g.ndim) * g.nown, memory, c->stream);
	dual_contour_whole(f, gr, g.ndim, g.gn, iso, c->stream, out);
}

}  // namespace fi
