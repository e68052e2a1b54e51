// fi_smooth.hip -- a device mesh made smoother by Taubin's lambda | mu fairing with uniform weights, and vertex normals
// recomputed from the primitives.
//
// The contract (include/fi_hip.h fi_mesh_smooth / fi_mesh_normals; tests/smooth_reference.py is its definition
// in numpy): every vertex moves towards the average of the set it averages over -- its distinct neighbours N(v), or its
// neighbours across boundary edges, or nothing, as the boundary mode says -- by the factor lambda, then by the factor mu; fp64
// from the fp32 coordinates, one rounding per operation (-ffp-contract=off), every sum serial in ascending order from 0.
// Nothing here depends on the run or the launch shape.
//
// How it is found:
//   rows       both directed pairs (v, w), (w, v) of every half-edge as keys v << bits | w, sorted (fi_prim.h's Onesweep, keys
//              only).  The head of a run of equal keys is a distinct neighbour; a run of one is a boundary edge (3-D); a
//              vertex with one key in all is a boundary vertex (2-D).  The heads the boundary mode keeps are flagged, scanned
//              and compacted into a CSR: uint32 offsets (a lower bound per vertex), uint32 neighbours.  The rows ARE the
//              averaging sets: a vertex that must not move has an empty row, and the step kernel knows no modes.
//   steps      one thread per vertex walks its row, sums the neighbours' fp64 positions in registers and writes the other
//              of two fp64 buffers; the last step of an iteration clamps, the last step of all casts to the output's fp32
//              positions.  Vertices are in key order (lattice order for an extracted mesh): neighbouring threads gather
//              neighbouring lines.
//   normals    (vertex, primitive) pairs, one per distinct vertex of a primitive, sorted by vertex (stable: a vertex's
//              primitives ascend); one thread per vertex sums the normals of its run.
// No floating-point atomics, no atomics writing an output (only the non-finite flag), no host synchronisation before the
// one at the end that reads that flag, one device allocation for every temporary of a call (fi_arena.h).
#include "fi_solver_internal.h"
#include "fi_smooth.h"
#include "fi_prim.h"

#include <algorithm>
#include <memory>

namespace fi {
namespace {

// ---- checks -----------------------------------------------------------------------------------------------------------

// every corner of every primitive: a vertex some primitive uses must be finite
template <int D>
__global__ __launch_bounds__(kThreads) void k_smooth_finite(int64_t n, const int* __restrict__ idx, const float* __restrict__ pos, uint32_t* err)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	const int64_t v      = idx[i];
	bool          finite = true;
#pragma unroll
	for (int d = 0; d < D; ++d) { finite = finite && isfinite(pos[v * D + d]); }
	if (!finite) { atomicOr(err, 1u); }
}

// ---- rows -------------------------------------------------------------------------------------------------------------

// both directions of every half-edge of primitive p, in slots 2 E p .. 2 E p + 2 E - 1 (E half-edges a primitive); a
// half-edge with equal ends: `sentinel` (above every key) twice
template <int D>
__global__ __launch_bounds__(kThreads) void k_smooth_pairs(int64_t np, int bits, uint64_t sentinel, const int* __restrict__ idx,
                                                            uint64_t* __restrict__ key)
{
	constexpr int E = D == 3 ? 3 : 1;
	const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (p >= np) { return; }
	uint64_t t[D];
#pragma unroll
	for (int k = 0; k < D; ++k) { t[k] = static_cast<uint64_t>(idx[p * D + k]); }
#pragma unroll
	for (int e = 0; e < E; ++e) {
		const uint64_t a = t[e], b = t[(e + 1) % D];
		key[(p * E + e) * 2]     = a == b ? sentinel : (a << bits) | b;
		key[(p * E + e) * 2 + 1] = a == b ? sentinel : (b << bits) | a;
	}
}

// what sorted slot s is: the head of a run of equal keys, and whether it stands alone -- 3-D: in its run (a boundary edge);
// 2-D: among the keys of its vertex (a vertex of total degree 1)
template <int D>
__device__ inline void slot_of(int64_t s, int64_t n, int bits, const uint64_t* __restrict__ key, uint64_t sentinel, uint64_t& k, bool& head,
                               bool& alone)
{
	k = key[s];
	const bool     first = s == 0, last = s + 1 == n;
	const uint64_t before = first ? 0 : key[s - 1], behind = last ? 0 : key[s + 1];
	head = k != sentinel && (first || before != k);
	if constexpr (D == 3) {
		alone = head && (last || behind != k);
	} else {
		alone = head && (first || (before >> bits) != (k >> bits)) && (last || (behind >> bits) != (k >> bits));
	}
}

// the boundary vertices (plain stores of the same 1: no atomics)
template <int D>
__global__ __launch_bounds__(kThreads) void k_smooth_boundary(int64_t n, int bits, const uint64_t* __restrict__ key, uint64_t sentinel,
                                                               uint32_t* __restrict__ vbnd)
{
	const int64_t s = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (s >= n) { return; }
	uint64_t k;
	bool     head, alone;
	slot_of<D>(s, n, bits, key, sentinel, k, head, alone);
	if (alone) { vbnd[k >> bits] = 1; }
}

// the heads that enter their vertex's row under the boundary mode (entry n: 0, the place of the scan's total)
template <int D>
__global__ __launch_bounds__(kThreads) void k_smooth_flags(int64_t n, int bits, const uint64_t* __restrict__ key, uint64_t sentinel, int mode,
                                                            const uint32_t* __restrict__ vbnd, uint32_t* __restrict__ flag)
{
	const int64_t s = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (s > n) { return; }
	bool keep = false;
	if (s < n) {
		uint64_t k;
		bool     head, alone;
		slot_of<D>(s, n, bits, key, sentinel, k, head, alone);
		keep = head;
		if (head && mode != FI_SMOOTH_BOUNDARY_FREE && vbnd[k >> bits]) {
			keep = D == 3 && mode == FI_SMOOTH_BOUNDARY_SLIDE && alone;  // a rim vertex slides along its boundary edges
		}
	}
	flag[s] = keep ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void k_smooth_compact(int64_t n, int bits, const uint64_t* __restrict__ key, const uint32_t* __restrict__ flag,
                                                              const uint32_t* __restrict__ number, uint32_t* __restrict__ nbr)
{
	const int64_t s = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (s >= n || !flag[s]) { return; }
	nbr[number[s]] = static_cast<uint32_t>(key[s] & ((uint64_t(1) << bits) - 1));
}

// start[v], v = 0 .. nv: the first sorted slot whose key is not below v << shift, or with `number` what the scan counted
// before that slot (number[n]: the total).  Unused vertices have no slot of their own: their rows come out empty.
__global__ __launch_bounds__(kThreads) void k_smooth_starts(int64_t nv, int64_t n, int shift, const uint64_t* __restrict__ key,
                                                             const uint32_t* __restrict__ number, uint32_t* __restrict__ start)
{
	const int64_t v = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (v > nv) { return; }
	const uint64_t want = static_cast<uint64_t>(v) << shift;
	int64_t        lo = 0, hi = n;
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (key[mid] < want) {
			lo = mid + 1;
		} else {
			hi = mid;
		}
	}
	start[v] = number ? number[lo] : static_cast<uint32_t>(lo);
}

// ---- steps ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_smooth_widen(int64_t n, const float* __restrict__ pos, double* __restrict__ x)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i < n) { x[i] = static_cast<double>(pos[i]); }
}

struct StepArgs {
	int64_t         nv;
	const uint32_t* off;   // uint32[nv + 1]
	const uint32_t* nbr;
	const double*   x;     // double[nv][D]: the positions before the step
	double          f;     // lambda or mu
	const float*    pos0;  // the input positions (CLAMP)
	double          m;     // max_move (CLAMP)
	double*         xo;    // double[nv][D]: the positions after it, or (CAST)
	float*          po;    // float[nv][D]: the output mesh's
};

// x' = x + f (avg - x) over the vertex's row; CLAMP: back to within m of the input position; CAST: the last step of all
template <int D, bool CLAMP, bool CAST>
__global__ __launch_bounds__(kThreads) void k_smooth_step(StepArgs a)
{
	const int64_t v = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (v >= a.nv) { return; }
	const uint32_t b = a.off[v], e = a.off[v + 1];
	double         x[D], s[D];
#pragma unroll
	for (int d = 0; d < D; ++d) {
		x[d] = a.x[v * D + d];
		s[d] = 0.0;
	}
	if (e > b) {
		for (uint32_t j = b; j < e; ++j) {
			const int64_t w = a.nbr[j];
#pragma unroll
			for (int d = 0; d < D; ++d) { s[d] = s[d] + a.x[w * D + d]; }
		}
		const double count = static_cast<double>(e - b);
#pragma unroll
		for (int d = 0; d < D; ++d) {
			double t = s[d] / count;
			t        = t - x[d];
			t        = a.f * t;
			x[d]     = x[d] + t;
		}
	}
	if constexpr (CLAMP) {
		double x0[D], dl[D];
#pragma unroll
		for (int d = 0; d < D; ++d) {
			x0[d] = static_cast<double>(a.pos0[v * D + d]);
			dl[d] = x[d] - x0[d];
		}
		double s2 = dl[0] * dl[0] + dl[1] * dl[1];
		if constexpr (D == 3) { s2 = s2 + dl[2] * dl[2]; }
		if (s2 > a.m * a.m) {
			const double r = a.m / sqrt(s2);
#pragma unroll
			for (int d = 0; d < D; ++d) { x[d] = x0[d] + dl[d] * r; }
		}
	}
#pragma unroll
	for (int d = 0; d < D; ++d) {
		if constexpr (CAST) {
			a.po[v * D + d] = static_cast<float>(x[d]);
		} else {
			a.xo[v * D + d] = x[d];
		}
	}
}

// ---- normals ----------------------------------------------------------------------------------------------------------

// one entry per distinct vertex of a primitive, in slot D p + k; a repeated vertex's slot sorts behind everything (key nv)
template <int D>
__global__ __launch_bounds__(kThreads) void k_smooth_incidence(int64_t np, int64_t nv, const int* __restrict__ idx, uint64_t* __restrict__ key,
                                                                uint32_t* __restrict__ val)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (p >= np) { return; }
	uint32_t t[D];
#pragma unroll
	for (int k = 0; k < D; ++k) { t[k] = static_cast<uint32_t>(idx[p * D + k]); }
#pragma unroll
	for (int k = 0; k < D; ++k) {
		bool again = false;
#pragma unroll
		for (int j = 0; j < k; ++j) { again = again || t[j] == t[k]; }
		key[p * D + k] = again ? static_cast<uint64_t>(nv) : t[k];
		val[p * D + k] = static_cast<uint32_t>(p);
	}
}

// the sum of the normals of the vertex's primitives, ascending, over its length
template <int D>
__global__ __launch_bounds__(kThreads) void k_smooth_normals(int64_t nv, const uint32_t* __restrict__ first, const uint32_t* __restrict__ porder,
                                                              const int* __restrict__ idx, const float* __restrict__ pos, float* __restrict__ nrm)
{
	const int64_t v = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (v >= nv) { return; }
	double s[D];
#pragma unroll
	for (int d = 0; d < D; ++d) { s[d] = 0.0; }
	const uint32_t b = first[v], e = first[v + 1];
	for (uint32_t j = b; j < e; ++j) {
		const int64_t p = porder[j];
		double        q[D][D];
#pragma unroll
		for (int k = 0; k < D; ++k) {
			const int64_t w = idx[p * D + k];
#pragma unroll
			for (int d = 0; d < D; ++d) { q[k][d] = static_cast<double>(pos[w * D + d]); }
		}
		if constexpr (D == 3) {
			double u[3], w[3];
#pragma unroll
			for (int d = 0; d < 3; ++d) {
				u[d] = q[1][d] - q[0][d];
				w[d] = q[2][d] - q[0][d];
			}
			s[0] = s[0] + (u[1] * w[2] - u[2] * w[1]);
			s[1] = s[1] + (u[2] * w[0] - u[0] * w[2]);
			s[2] = s[2] + (u[0] * w[1] - u[1] * w[0]);
		} else {
			s[0] = s[0] + (q[1][1] - q[0][1]);
			s[1] = s[1] + -(q[1][0] - q[0][0]);
		}
	}
	double l2 = s[0] * s[0] + s[1] * s[1];
	if constexpr (D == 3) { l2 = l2 + s[2] * s[2]; }
	const double len = sqrt(l2);
#pragma unroll
	for (int d = 0; d < D; ++d) { nrm[v * D + d] = len > 0.0 ? static_cast<float>(s[d] / len) : 0.0f; }
}

// ---- host side --------------------------------------------------------------------------------------------------------

using namespace prim;  // Arena, Scratch, scan_u32, sort_u64, sort_keys, read_u32, bits_for, grid
static_assert(kThreads == kGridThreads, "grid() counts work groups of kThreads");

// the temporaries of a call; the pieces of a stage the call does not run are not taken
struct Work {
	// zeroed before use, as one range
	uint32_t *err, *vbnd;
	size_t    zeroed;
	// rows
	uint64_t *key, *key2;
	uint32_t *flag, *number, *nbr, *off;
	double *  xa, *xb;
	// normals
	uint64_t *ikey, *ikey2;
	uint32_t *ival, *porder, *first;
	Scratch   tmp;
};

struct Plan {
	int64_t nv, np, pairs, corners;  // pairs: directed vertex pairs (rows); corners: primitive corners (normals)
	int     bits;                     // of a vertex number
	bool    steps, normals;
};

void lay_out(Arena& a, const Plan& p, int D, size_t tmp_bytes, Work& w)
{
	w.err    = a.take<uint32_t>(1);
	w.vbnd   = p.steps ? a.take<uint32_t>(p.nv) : nullptr;
	w.zeroed = a.bytes();
	if (p.steps) {
		w.key    = a.take<uint64_t>(p.pairs);
		w.key2   = a.take<uint64_t>(p.pairs);
		w.flag   = a.take<uint32_t>(p.pairs + 1);
		w.number = a.take<uint32_t>(p.pairs + 1);
		w.nbr    = a.take<uint32_t>(p.pairs);
		w.off    = a.take<uint32_t>(p.nv + 1);
		w.xa     = a.take<double>(p.nv * D);
		w.xb     = a.take<double>(p.nv * D);
	}
	if (p.normals) {
		w.ikey   = a.take<uint64_t>(p.corners);
		w.ikey2  = a.take<uint64_t>(p.corners);
		w.ival   = a.take<uint32_t>(p.corners);
		w.porder = a.take<uint32_t>(p.corners);
		w.first  = a.take<uint32_t>(p.nv + 1);
	}
	w.tmp.p     = a.take<char>(static_cast<int64_t>(tmp_bytes));
	w.tmp.bytes = tmp_bytes;
}

template <int D>
void build_rows(const Plan& p, const int* idx, int mode, const Work& w, hipStream_t st)
{
	const int64_t  n        = p.pairs;
	const uint64_t sentinel = static_cast<uint64_t>(p.nv) << p.bits;
	hipLaunchKernelGGL(k_smooth_pairs<D>, grid(p.np), dim3(kThreads), 0, st, p.np, p.bits, sentinel, idx, w.key);
	FI_HIP_TRY(hipGetLastError());
	sort_keys(w.key, w.key2, n, 0, p.bits + bits_for(p.nv + 1), w.tmp, st);
	if (mode != FI_SMOOTH_BOUNDARY_FREE) {
		hipLaunchKernelGGL(k_smooth_boundary<D>, grid(n), dim3(kThreads), 0, st, n, p.bits, w.key2, sentinel, w.vbnd);
	}
	hipLaunchKernelGGL(k_smooth_flags<D>, grid(n + 1), dim3(kThreads), 0, st, n, p.bits, w.key2, sentinel, mode, w.vbnd, w.flag);
	FI_HIP_TRY(hipGetLastError());
	scan_u32(w.flag, w.number, n + 1, w.tmp, st);
	hipLaunchKernelGGL(k_smooth_compact, grid(n), dim3(kThreads), 0, st, n, p.bits, w.key2, w.flag, w.number, w.nbr);
	hipLaunchKernelGGL(k_smooth_starts, grid(p.nv + 1), dim3(kThreads), 0, st, p.nv, n, p.bits, w.key2, w.number, w.off);
	FI_HIP_TRY(hipGetLastError());
}

template <int D>
void run_steps(const Plan& p, const fi_smooth_options& opt, const float* pos, const Work& w, float* pos_out, hipStream_t st)
{
	hipLaunchKernelGGL(k_smooth_widen, grid(p.nv * D), dim3(kThreads), 0, st, p.nv * D, pos, w.xa);
	const bool second = opt.mu != 0.0f, clamped = opt.max_move > 0.0f;
	const int  per    = second ? 2 : 1;
	double *   from = w.xa, *to = w.xb;
	StepArgs   a{};
	a.nv   = p.nv;
	a.off  = w.off;
	a.nbr  = w.nbr;
	a.pos0 = pos;
	a.m    = static_cast<double>(opt.max_move);
	a.po   = pos_out;
	for (int it = 0; it < opt.iterations; ++it) {
		for (int k = 0; k < per; ++k) {
			const bool clamp = clamped && k == per - 1, cast = it == opt.iterations - 1 && k == per - 1;
			a.x  = from;
			a.xo = to;
			a.f  = static_cast<double>(k == 0 ? opt.lambda : opt.mu);
			if (clamp && cast) {
				hipLaunchKernelGGL((k_smooth_step<D, true, true>), grid(p.nv), dim3(kThreads), 0, st, a);
			} else if (clamp) {
				hipLaunchKernelGGL((k_smooth_step<D, true, false>), grid(p.nv), dim3(kThreads), 0, st, a);
			} else if (cast) {
				hipLaunchKernelGGL((k_smooth_step<D, false, true>), grid(p.nv), dim3(kThreads), 0, st, a);
			} else {
				hipLaunchKernelGGL((k_smooth_step<D, false, false>), grid(p.nv), dim3(kThreads), 0, st, a);
			}
			std::swap(from, to);
		}
	}
	FI_HIP_TRY(hipGetLastError());
}

template <int D>
void run_normals(const Plan& p, const int* idx, const float* pos, const Work& w, float* nrm, hipStream_t st)
{
	const int64_t n = p.corners;
	hipLaunchKernelGGL(k_smooth_incidence<D>, grid(p.np), dim3(kThreads), 0, st, p.np, p.nv, idx, w.ikey, w.ival);
	FI_HIP_TRY(hipGetLastError());
	sort_u64(w.ikey, w.ikey2, w.ival, w.porder, n, 0, bits_for(p.nv + 1), w.tmp, st);
	hipLaunchKernelGGL(k_smooth_starts, grid(p.nv + 1), dim3(kThreads), 0, st, p.nv, n, 0, w.ikey2, static_cast<const uint32_t*>(nullptr), w.first);
	hipLaunchKernelGGL(k_smooth_normals<D>, grid(p.nv), dim3(kThreads), 0, st, p.nv, w.first, w.porder, idx, pos, nrm);
	FI_HIP_TRY(hipGetLastError());
}

// o: the input's sizes, keys and indices already there; steps: opt's iterations run (else the positions are copied);
// normals: o's normals are computed from o's positions
template <int D>
void run(const fi_mesh* m, const fi_smooth_options& opt, bool steps, bool normals, fi_mesh* o, hipStream_t st)
{
	Plan p{};
	p.nv      = m->nv;
	p.np      = m->np;
	p.pairs   = m->np * (D == 3 ? 6 : 2);
	p.corners = m->np * D;
	p.bits    = bits_for(m->nv);
	p.steps   = steps;
	p.normals = normals;
	FI_REQUIRE(p.pairs < (int64_t(1) << 32), FI_ERR_UNSUPPORTED, "the mesh has %lld directed vertex pairs", static_cast<long long>(p.pairs));
	const int*   idx = m->idx.as<int>();
	const float* pos = m->pos.as<float>();

	size_t tmp_bytes = 0;
	if (steps) { tmp_bytes = std::max(sort_keys_bytes(p.pairs, 0, p.bits + bits_for(p.nv + 1)), scan_bytes(p.pairs + 1)); }
	if (normals) { tmp_bytes = std::max(tmp_bytes, sort_bytes(p.corners, 0, bits_for(p.nv + 1))); }
	Work   w{};
	DevBuf block;
	arena_alloc(block, [&](Arena& a) { lay_out(a, p, D, tmp_bytes, w); });
	FI_HIP_TRY(hipMemsetAsync(block.p, 0, w.zeroed, st));

	hipLaunchKernelGGL(k_smooth_finite<D>, grid(p.corners), dim3(kThreads), 0, st, p.corners, idx, pos, w.err);
	FI_HIP_TRY(hipGetLastError());
	if (steps) {
		build_rows<D>(p, idx, opt.boundary, w, st);
		run_steps<D>(p, opt, pos, w, o->pos.as<float>(), st);
	} else {
		FI_HIP_TRY(hipMemcpyAsync(o->pos.p, m->pos.p, sizeof(float) * D * p.nv, hipMemcpyDeviceToDevice, st));
	}
	if (normals) { run_normals<D>(p, idx, o->pos.as<float>(), w, o->nrm.as<float>(), st); }
	const uint32_t bad = read_u32(w.err, st);  // (the call's one synchronisation)
	FI_REQUIRE(bad == 0, FI_ERR_INVALID, "a vertex the mesh uses has a non-finite coordinate");
}

enum class Normals { none, copy, compute };

// the new mesh of both entries: m's keys and indices, positions after opt's iterations (iterations 0: m's), normals as said
void make(const fi_mesh* m, const fi_smooth_options& opt, Normals normals, fi_mesh** out)
{
	FI_REQUIRE(m->ndim == 2 || m->ndim == 3, FI_ERR_INVALID, "a mesh of %d-vertex primitives", m->ndim);
	FI_HIP_TRY(hipSetDevice(m->device));
	std::unique_ptr<fi_mesh> o(new fi_mesh());
	o->device      = m->device;
	o->ndim        = m->ndim;
	o->has_normals = normals != Normals::none;
	o->nv          = m->nv;
	o->np          = m->np;
	hipStream_t  st = nullptr;
	const size_t D  = static_cast<size_t>(m->ndim);
	if (m->nv > 0) {
		const size_t vbytes = sizeof(float) * D * static_cast<size_t>(m->nv);
		o->pos.alloc(vbytes);
		o->key.alloc(sizeof(int64_t) * m->nv);
		o->idx.alloc(sizeof(int) * D * (m->np > 0 ? m->np : 1));
		FI_HIP_TRY(hipMemcpyAsync(o->key.p, m->key.p, sizeof(int64_t) * m->nv, hipMemcpyDeviceToDevice, st));
		if (m->np > 0) { FI_HIP_TRY(hipMemcpyAsync(o->idx.p, m->idx.p, sizeof(int) * D * m->np, hipMemcpyDeviceToDevice, st)); }
		if (normals != Normals::none) { o->nrm.alloc(vbytes); }
		if (normals == Normals::copy) { FI_HIP_TRY(hipMemcpyAsync(o->nrm.p, m->nrm.p, vbytes, hipMemcpyDeviceToDevice, st)); }
		if (m->np > 0) {
			// (without primitives no vertex is used: none moves, every normal is zero)
			if (m->ndim == 2) {
				run<2>(m, opt, opt.iterations > 0, normals == Normals::compute, o.get(), st);
			} else {
				run<3>(m, opt, opt.iterations > 0, normals == Normals::compute, o.get(), st);
			}
		} else {
			FI_HIP_TRY(hipMemcpyAsync(o->pos.p, m->pos.p, vbytes, hipMemcpyDeviceToDevice, st));
			if (normals == Normals::compute) { FI_HIP_TRY(hipMemsetAsync(o->nrm.p, 0, vbytes, st)); }
			FI_HIP_TRY(hipStreamSynchronize(st));
		}
	}
	*out = o.release();
}

}  // namespace

void mesh_smooth(const fi_mesh* m, const fi_smooth_options* opt, fi_mesh** out)
{
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "out is null");
	*out = nullptr;
	FI_REQUIRE(m != nullptr, FI_ERR_INVALID, "null mesh");
	FI_REQUIRE(opt != nullptr, FI_ERR_INVALID, "null options");
	FI_REQUIRE(opt->iterations >= 0, FI_ERR_INVALID, "iterations must be >= 0 (got %d)", opt->iterations);
	// (every comparison is false for a NaN)
	FI_REQUIRE(opt->lambda >= 0.0f && opt->lambda <= 1.0f, FI_ERR_INVALID, "lambda must lie in [0, 1] (got %g)", static_cast<double>(opt->lambda));
	FI_REQUIRE(opt->mu >= -2.0f && opt->mu <= 0.0f, FI_ERR_INVALID, "mu must lie in [-2, 0] (got %g)", static_cast<double>(opt->mu));
	FI_REQUIRE(opt->max_move >= 0.0f, FI_ERR_INVALID, "max_move must be >= 0 (got %g)", static_cast<double>(opt->max_move));
	FI_REQUIRE(opt->boundary == FI_SMOOTH_BOUNDARY_FIXED || opt->boundary == FI_SMOOTH_BOUNDARY_SLIDE || opt->boundary == FI_SMOOTH_BOUNDARY_FREE,
	           FI_ERR_INVALID, "bad boundary mode %d", opt->boundary);
	FI_REQUIRE(opt->normals == FI_SMOOTH_NORMALS_RECOMPUTE || opt->normals == FI_SMOOTH_NORMALS_KEEP, FI_ERR_INVALID, "bad normals mode %d",
	           opt->normals);
	const Normals normals = !m->has_normals ? Normals::none : opt->normals == FI_SMOOTH_NORMALS_KEEP ? Normals::copy : Normals::compute;
	make(m, *opt, normals, out);
}

void mesh_normals(const fi_mesh* m, fi_mesh** out)
{
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "out is null");
	*out = nullptr;
	FI_REQUIRE(m != nullptr, FI_ERR_INVALID, "null mesh");
	fi_smooth_options none{};  // (no iterations: the positions are the input's)
	make(m, none, Normals::compute, out);
}

}  // namespace fi
