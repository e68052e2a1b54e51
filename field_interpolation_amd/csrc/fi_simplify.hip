// fi_simplify.hip -- a device mesh made coarser (or a triangle soup welded) by vertex clustering on a uniform grid, each
// cluster's vertex placed at the minimum of its quadric error function or at its mean.
//
// The contract (include/fi_hip.h fi_mesh_simplify; tests/simplify_reference.py is its definition in numpy):
// the cell of a used vertex in fp32, clusters = the distinct cell keys ascending, primitives remapped to clusters with the
// degenerate ones and all but the lowest of every oriented tuple dropped, output vertices = the clusters a survivor uses;
// placement in fp64 relative to the cell centre, one rounding per operation (-ffp-contract=off), every sum serial in
// ascending order.  Nothing here depends on the run or the launch shape.
//
// How it is found:
//   clusters   (cell key, vertex) pairs sorted by key (fi_prim.h's Onesweep, stable: a cluster's vertices ascend); unused
//              vertices carry a key above every cell's and end up behind.  Run heads scanned into cluster numbers.
//   dedupe     every primitive's canonical cluster triple sorted by two stable passes (the last two entries, then the first:
//              3 x 31 bits do not fit one key); the head of a run of equal triples is its lowest primitive and sets that
//              primitive's keep flag.  Kept primitives flag their clusters; two scans number what stays.
//   placement  QUADRIC: (cluster, primitive) pairs, one per distinct cluster of a primitive, sorted by cluster (stable: a
//              cluster's primitives ascend).  One thread per surviving cluster walks its vertex run (mean, normal sum) and
//              its primitive run (A, b), solves the 3 x 3 (2 x 2) system by the Jacobi iteration of fi_jacobi.h, and writes
//              the cluster's position and normal.  Neighbouring clusters are neighbours in x: their gathers share lines.
//   gather     surviving clusters and primitives to their scanned places, indices remapped; the vertex map.
// No floating-point atomics, no atomics writing an output, one read-back per size the host needs, one device allocation for
// every temporary of a call (fi_arena.h; the host helpers around the sorts and scans are fi_prim.h's).
#include "fi_solver_internal.h"
#include "fi_stage.h"
#include "fi_simplify.h"
#include "fi_prim.h"
#include "fi_jacobi.h"

#include <algorithm>
#include <memory>

namespace fi {
namespace {

constexpr int      kCellBias    = 1 << 20;  // |cell coordinate| < 2^20: 21 bits an axis
constexpr double   kRankCut     = 1e-3;     // eigenvalues <= kRankCut * the largest take no part in the minimiser
constexpr uint32_t kErrNonFinite = 1u, kErrRange = 2u;

struct Grid {
	float cell;
	float o[3];
};

// ---- clusters ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_simp_mark(int64_t n, const int* __restrict__ idx, uint32_t* __restrict__ used)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i < n) { used[idx[i]] = 1; }
}

// the cell key of every used vertex; `sentinel` (above every key) for the others
template <int D>
__global__ __launch_bounds__(kThreads) void k_simp_keys(int64_t nv, const float* __restrict__ pos, const uint32_t* __restrict__ used, Grid g,
                                                         uint64_t sentinel, uint64_t* __restrict__ key, uint32_t* __restrict__ val,
                                                         uint32_t* err)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= nv) { return; }
	val[i] = static_cast<uint32_t>(i);
	uint64_t k = sentinel;
	if (used[i]) {
		bool finite = true, inside = true;
		k = 0;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			const float p = pos[i * D + d];
			const float c = floorf((p - g.o[d]) / g.cell);
			finite        = finite && isfinite(p);
			const bool in = fabsf(c) < static_cast<float>(kCellBias);  // (false for a NaN)
			inside        = inside && in;
			k |= static_cast<uint64_t>((in ? static_cast<int>(c) : 0) + kCellBias) << (21 * d);
		}
		if (!finite) {
			atomicOr(err, kErrNonFinite);
		} else if (!inside) {
			atomicOr(err, kErrRange);
		}
		if (!finite || !inside) { k = sentinel; }
	}
	key[i] = k;
}

__global__ __launch_bounds__(kThreads) void k_simp_heads(int64_t nv, const uint64_t* __restrict__ key, uint64_t sentinel,
                                                          uint32_t* __restrict__ head)
{
	const int64_t s = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (s > nv) { return; }
	head[s] = s < nv && key[s] != sentinel && (s == 0 || key[s - 1] != key[s]) ? 1u : 0u;  // (entry nv: the scan's total)
}

// every used vertex's cluster; every cluster's key and the start of its run of sorted vertices (first[nc]: the end of the last)
__global__ __launch_bounds__(kThreads) void k_simp_assign(int64_t nv, int64_t nc, const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                           const uint32_t* __restrict__ head, const uint32_t* __restrict__ number,
                                                           uint64_t sentinel, int* __restrict__ vcl, uint32_t* __restrict__ first,
                                                           long long* __restrict__ ckey)
{
	const int64_t s = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (s > nv) { return; }
	if (s < nv && key[s] != sentinel) {
		const uint32_t c = number[s] + head[s] - 1u;
		vcl[val[s]] = static_cast<int>(c);
		if (head[s]) {
			first[c] = static_cast<uint32_t>(s);
			ckey[c]  = static_cast<long long>(key[s]);
		}
	} else {
		if (s < nv) { vcl[val[s]] = -1; }
		if (s == 0 || key[s - 1] != sentinel) { first[nc] = static_cast<uint32_t>(s); }
	}
}

// ---- primitives ---------------------------------------------------------------------------------------------------------

// primitive p in cluster numbers, as its oriented tuple: 3-D rotated so that the smallest comes first, 2-D as it is (t[2] = 0)
template <int D>
__device__ inline bool tuple_of(const int* __restrict__ idx, const int* __restrict__ vcl, int64_t p, uint32_t (&t)[3])
{
	uint32_t r[3] = {0, 0, 0};
#pragma unroll
	for (int k = 0; k < D; ++k) { r[k] = static_cast<uint32_t>(vcl[idx[p * D + k]]); }
	if constexpr (D == 3) {
		const bool degenerate = r[0] == r[1] || r[1] == r[2] || r[0] == r[2];
		if (r[0] <= r[1] && r[0] <= r[2]) {
			t[0] = r[0], t[1] = r[1], t[2] = r[2];
		} else if (r[1] <= r[2]) {
			t[0] = r[1], t[1] = r[2], t[2] = r[0];
		} else {
			t[0] = r[2], t[1] = r[0], t[2] = r[1];
		}
		return degenerate;
	} else {
		t[0] = r[0], t[1] = r[1], t[2] = 0;
		return r[0] == r[1];
	}
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_simp_tuple_low(int64_t np, int cbits, const int* __restrict__ idx, const int* __restrict__ vcl,
                                                              uint64_t* __restrict__ key, uint32_t* __restrict__ val)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (p >= np) { return; }
	uint32_t t[3];
	tuple_of<D>(idx, vcl, p, t);
	key[p] = D == 3 ? (static_cast<uint64_t>(t[1]) << cbits) | t[2] : t[1];
	val[p] = static_cast<uint32_t>(p);
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_simp_tuple_high(int64_t np, const uint32_t* __restrict__ order, const int* __restrict__ idx,
                                                               const int* __restrict__ vcl, uint64_t* __restrict__ key)
{
	const int64_t s = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (s >= np) { return; }
	uint32_t t[3];
	tuple_of<D>(idx, vcl, order[s], t);
	key[s] = t[0];
}

// the sorted primitives: the first of a run of equal tuples is the run's lowest primitive; it stays unless it is degenerate
template <int D>
__global__ __launch_bounds__(kThreads) void k_simp_keep(int64_t np, const uint32_t* __restrict__ order, const int* __restrict__ idx,
                                                         const int* __restrict__ vcl, uint32_t* __restrict__ keep)
{
	const int64_t s = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (s >= np) { return; }
	uint32_t   t[3], q[3];
	const bool degenerate = tuple_of<D>(idx, vcl, order[s], t);
	bool       head       = s == 0;
	if (!head) {
		tuple_of<D>(idx, vcl, order[s - 1], q);
		head = q[0] != t[0] || q[1] != t[1] || q[2] != t[2];
	}
	if (head && !degenerate) { keep[order[s]] = 1; }
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_simp_cluster_flags(int64_t np, const uint32_t* __restrict__ keep, const int* __restrict__ idx,
                                                                  const int* __restrict__ vcl, uint32_t* __restrict__ cused)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (p >= np || !keep[p]) { return; }
#pragma unroll
	for (int k = 0; k < D; ++k) { cused[vcl[idx[p * D + k]]] = 1; }
}

// ---- placement ----------------------------------------------------------------------------------------------------------

// one entry per distinct cluster of a primitive, in slot D p + k; a repeated cluster's slot sorts behind everything (key nc)
template <int D>
__global__ __launch_bounds__(kThreads) void k_simp_pairs(int64_t np, int64_t nc, const int* __restrict__ idx, const int* __restrict__ vcl,
                                                          uint64_t* __restrict__ key, uint32_t* __restrict__ val)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (p >= np) { return; }
	uint32_t t[D];
#pragma unroll
	for (int k = 0; k < D; ++k) { t[k] = static_cast<uint32_t>(vcl[idx[p * D + k]]); }
#pragma unroll
	for (int k = 0; k < D; ++k) {
		bool again = false;
#pragma unroll
		for (int j = 0; j < k; ++j) { again = again || t[j] == t[k]; }
		key[p * D + k] = again ? static_cast<uint64_t>(nc) : t[k];
		val[p * D + k] = static_cast<uint32_t>(p);
	}
}

// first[c]: where cluster c begins in the sorted pairs (every cluster has one); first[nc]: where the repeated slots begin
__global__ __launch_bounds__(kThreads) void k_simp_pair_first(int64_t n, int64_t nc, const uint64_t* __restrict__ key, uint32_t* __restrict__ first)
{
	const int64_t s = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (s > n) { return; }
	const uint64_t k = s < n ? key[s] : static_cast<uint64_t>(nc);
	if (s == 0 || key[s - 1] != k) { first[k] = static_cast<uint32_t>(s); }
}

struct PlaceArgs {
	int64_t          nc;
	Grid             g;
	const uint32_t*  cused;    // uint32[nc]: clusters without a surviving primitive are skipped
	const long long* ckey;     // int64[nc]
	const uint32_t*  vfirst;   // uint32[nc + 1] into vorder
	const uint32_t*  vorder;   // the used vertices by cluster, ascending within one
	const uint32_t*  pfirst;   // uint32[nc + 1] into porder (QUADRIC)
	const uint32_t*  porder;   // the primitives by cluster, ascending within one
	const int*       idx;
	const float*     pos;
	const float*     nrm;      // or nullptr
	float*           cpos;     // float[nc][D]
	float*           cnrm;     // float[nc][D], or nullptr
};

template <int D, bool QUADRIC>
__global__ __launch_bounds__(kThreads) void k_simp_place(PlaceArgs a)
{
	const int64_t c = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (c >= a.nc || !a.cused[c]) { return; }
	const uint64_t key  = static_cast<uint64_t>(a.ckey[c]);
	const double   cell = static_cast<double>(a.g.cell);
	double         g[D], sx[D], sn[D];
#pragma unroll
	for (int d = 0; d < D; ++d) {
		const int ci = static_cast<int>((key >> (21 * d)) & 0x1FFFFFu) - kCellBias;
		g[d]  = static_cast<double>(a.g.o[d]) + (static_cast<double>(ci) + 0.5) * cell;
		sx[d] = 0.0;
		sn[d] = 0.0;
	}
	const uint32_t vb = a.vfirst[c], ve = a.vfirst[c + 1];
	for (uint32_t s = vb; s < ve; ++s) {
		const int64_t v = a.vorder[s];
#pragma unroll
		for (int d = 0; d < D; ++d) {
			sx[d] = sx[d] + (static_cast<double>(a.pos[v * D + d]) - g[d]);
			if (a.nrm) { sn[d] = sn[d] + static_cast<double>(a.nrm[v * D + d]); }
		}
	}
	const double count = static_cast<double>(ve - vb);
	double       mean[D], x[D];
#pragma unroll
	for (int d = 0; d < D; ++d) {
		mean[d] = sx[d] / count;
		x[d]    = mean[d];
	}
	if constexpr (QUADRIC) {
		double A[D][D], V[D][D], b[D];
#pragma unroll
		for (int i = 0; i < D; ++i) {
			b[i] = 0.0;
#pragma unroll
			for (int j = 0; j < D; ++j) {
				A[i][j] = 0.0;
				V[i][j] = i == j ? 1.0 : 0.0;
			}
		}
		const uint32_t pb = a.pfirst[c], pe = a.pfirst[c + 1];
		for (uint32_t s = pb; s < pe; ++s) {
			const int64_t p = a.porder[s];
			double        q[D][D];
#pragma unroll
			for (int k = 0; k < D; ++k) {
				const int64_t v = a.idx[p * D + k];
#pragma unroll
				for (int d = 0; d < D; ++d) { q[k][d] = static_cast<double>(a.pos[v * D + d]) - g[d]; }
			}
			double n[D], na;
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
				na   = (n[0] * q[0][0] + n[1] * q[0][1]) + n[2] * q[0][2];
			} else {
				n[0] = -(q[1][1] - q[0][1]);
				n[1] = q[1][0] - q[0][0];
				na   = n[0] * q[0][0] + n[1] * q[0][1];
			}
#pragma unroll
			for (int i = 0; i < D; ++i) {
				b[i] = b[i] + n[i] * na;
#pragma unroll
				for (int j = i; j < D; ++j) { A[i][j] = A[i][j] + n[i] * n[j]; }
			}
		}
#pragma unroll
		for (int i = 0; i < D; ++i) {
#pragma unroll
			for (int j = 0; j < i; ++j) { A[i][j] = A[j][i]; }
		}
		// the residual b - A mean, before the iteration takes A apart
		double r[D];
#pragma unroll
		for (int i = 0; i < D; ++i) {
			double t = A[i][0] * mean[0];
#pragma unroll
			for (int j = 1; j < D; ++j) { t = t + A[i][j] * mean[j]; }
			r[i] = b[i] - t;
		}
		jacobi::jacobi_sweeps<D>(A, V);
		double lmax = A[0][0];
#pragma unroll
		for (int i = 1; i < D; ++i) { lmax = A[i][i] > lmax ? A[i][i] : lmax; }
#pragma unroll
		for (int i = 0; i < D; ++i) {
			if (lmax > 0.0 && A[i][i] > kRankCut * lmax) {
				double dot = V[0][i] * r[0];
#pragma unroll
				for (int d = 1; d < D; ++d) { dot = dot + V[d][i] * r[d]; }
				const double coef = dot / A[i][i];
#pragma unroll
				for (int d = 0; d < D; ++d) { x[d] = x[d] + V[d][i] * coef; }
			}
		}
		bool bad = false;
#pragma unroll
		for (int d = 0; d < D; ++d) { bad = bad || !isfinite(x[d]) || fabs(x[d]) > cell; }
		if (bad) {
#pragma unroll
			for (int d = 0; d < D; ++d) { x[d] = mean[d]; }
		}
	}
#pragma unroll
	for (int d = 0; d < D; ++d) { a.cpos[c * D + d] = static_cast<float>(g[d] + x[d]); }
	if (a.cnrm) {
		double l2 = sn[0] * sn[0];
#pragma unroll
		for (int d = 1; d < D; ++d) { l2 = l2 + sn[d] * sn[d]; }
		const double len = sqrt(l2);
#pragma unroll
		for (int d = 0; d < D; ++d) { a.cnrm[c * D + d] = len > 0.0 ? static_cast<float>(sn[d] / len) : 0.0f; }
	}
}

// ---- gather -------------------------------------------------------------------------------------------------------------

template <int D>
__global__ __launch_bounds__(kThreads) void k_simp_gather_vertices(int64_t nc, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ to,
                                                                    const float* __restrict__ cpos, const float* __restrict__ cnrm,
                                                                    const long long* __restrict__ ckey, float* __restrict__ pos_out,
                                                                    float* __restrict__ nrm_out, long long* __restrict__ key_out)
{
	const int64_t c = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (c >= nc || !flag[c]) { return; }
	const int64_t j = to[c];
#pragma unroll
	for (int d = 0; d < D; ++d) {
		pos_out[j * D + d] = cpos[c * D + d];
		if (cnrm) { nrm_out[j * D + d] = cnrm[c * D + d]; }
	}
	key_out[j] = ckey[c];
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_simp_gather_prims(int64_t np, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ to,
                                                                 const uint32_t* __restrict__ cluster_to, const int* __restrict__ idx,
                                                                 const int* __restrict__ vcl, int* __restrict__ idx_out)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (p >= np || !flag[p]) { return; }
	const int64_t q = to[p];
#pragma unroll
	for (int k = 0; k < D; ++k) { idx_out[q * D + k] = static_cast<int>(cluster_to[vcl[idx[p * D + k]]]); }
}

// cused == nullptr: nothing survived
__global__ __launch_bounds__(kThreads) void k_simp_vertex_map(int64_t nv, const int* __restrict__ vcl, const uint32_t* __restrict__ cused,
                                                               const uint32_t* __restrict__ cluster_to, int* __restrict__ map)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= nv) { return; }
	const int c = cused ? vcl[i] : -1;
	map[i] = c >= 0 && cused[c] ? static_cast<int>(cluster_to[c]) : -1;
}

// ---- host side ----------------------------------------------------------------------------------------------------------

using namespace prim;  // Arena, Scratch, scan_u32, sort_u64, read_u32, bits_for, grid
static_assert(kThreads == kGridThreads, "grid() counts work groups of kThreads");

// the temporaries of a call; what depends on the number of clusters has room for one cluster per vertex
struct Work {
	// zeroed before use, as one range
	uint32_t *used, *err, *keep, *cused;
	size_t    zeroed;
	// clusters
	uint64_t *key, *key2;
	uint32_t *val, *vorder, *head, *number, *vfirst;
	int*      vcl;
	long long* ckey;
	// primitives
	uint64_t *tkey, *tkey2;
	uint32_t *tval, *tval2, *pto, *cto;
	// placement
	uint64_t *pkey, *pkey2;
	uint32_t *pval, *porder, *pfirst;
	float *   cpos, *cnrm;
	Scratch   tmp;
};

template <int D>
void lay_out(Arena& a, int64_t nv, int64_t np, bool quadric, bool normals, size_t tmp_bytes, Work& w)
{
	w.used   = a.take<uint32_t>(nv);
	w.err    = a.take<uint32_t>(1);
	w.keep   = a.take<uint32_t>(np + 1);
	w.cused  = a.take<uint32_t>(nv + 1);
	w.zeroed = a.bytes();
	w.key    = a.take<uint64_t>(nv);
	w.key2   = a.take<uint64_t>(nv);
	w.val    = a.take<uint32_t>(nv);
	w.vorder = a.take<uint32_t>(nv);
	w.head   = a.take<uint32_t>(nv + 1);
	w.number = a.take<uint32_t>(nv + 1);
	w.vfirst = a.take<uint32_t>(nv + 1);
	w.vcl    = a.take<int>(nv);
	w.ckey   = a.take<long long>(nv + 1);
	w.tkey   = a.take<uint64_t>(np);
	w.tkey2  = a.take<uint64_t>(np);
	w.tval   = a.take<uint32_t>(np);
	w.tval2  = a.take<uint32_t>(np);
	w.pto    = a.take<uint32_t>(np + 1);
	w.cto    = a.take<uint32_t>(nv + 1);
	w.pkey   = quadric ? a.take<uint64_t>(np * D) : nullptr;
	w.pkey2  = quadric ? a.take<uint64_t>(np * D) : nullptr;
	w.pval   = quadric ? a.take<uint32_t>(np * D) : nullptr;
	w.porder = quadric ? a.take<uint32_t>(np * D) : nullptr;
	w.pfirst = quadric ? a.take<uint32_t>(nv + 1) : nullptr;
	w.cpos   = a.take<float>(nv * D);
	w.cnrm   = normals ? a.take<float>(nv * D) : nullptr;
	w.tmp.p     = a.take<char>(static_cast<int64_t>(tmp_bytes));
	w.tmp.bytes = tmp_bytes;
}

template <int D>
void simplify(const fi_mesh* m, const Grid& g, bool quadric, int* dmap, fi_mesh* o, hipStream_t st)
{
	const int64_t  nv = m->nv, np = m->np;
	const int*     idx      = m->idx.as<int>();
	const float*   pos      = m->pos.as<float>();
	const float*   nrm      = m->has_normals ? m->nrm.as<float>() : nullptr;
	const uint64_t sentinel = uint64_t(1) << (21 * D);
	const int      vbits    = bits_for(nv);  // at most nv clusters
	FI_REQUIRE(np * D < (int64_t(1) << 32), FI_ERR_UNSUPPORTED, "the mesh has %lld primitive corners", static_cast<long long>(np * D));

	// the workspace of the largest primitive call, then everything in one block
	size_t tmp_bytes = std::max(sort_bytes(nv, 0, 21 * D + 1), std::max(sort_bytes(np, 0, 2 * vbits), scan_bytes(std::max(nv, np) + 1)));
	if (quadric) { tmp_bytes = std::max(tmp_bytes, sort_bytes(np * D, 0, bits_for(nv + 1))); }
	Work   w{};
	DevBuf block;
	arena_alloc(block, [&](Arena& a) { lay_out<D>(a, nv, np, quadric, nrm != nullptr, tmp_bytes, w); });
	FI_HIP_TRY(hipMemsetAsync(block.p, 0, w.zeroed, st));

	// clusters
	hipLaunchKernelGGL(k_simp_mark, grid(np * D), dim3(kThreads), 0, st, np * D, idx, w.used);
	hipLaunchKernelGGL(k_simp_keys<D>, grid(nv), dim3(kThreads), 0, st, nv, pos, w.used, g, sentinel, w.key, w.val, w.err);
	FI_HIP_TRY(hipGetLastError());
	sort_u64(w.key, w.key2, w.val, w.vorder, nv, 0, 21 * D + 1, w.tmp, st);
	hipLaunchKernelGGL(k_simp_heads, grid(nv + 1), dim3(kThreads), 0, st, nv, w.key2, sentinel, w.head);
	FI_HIP_TRY(hipGetLastError());
	scan_u32(w.head, w.number, nv + 1, w.tmp, st);
	const uint32_t bad = read_u32(w.err, st);
	FI_REQUIRE((bad & kErrNonFinite) == 0, FI_ERR_INVALID, "a vertex the mesh uses has a non-finite coordinate");
	FI_REQUIRE((bad & kErrRange) == 0, FI_ERR_INVALID, "a vertex lies 2^20 cells or more from the origin (cell %g)", static_cast<double>(g.cell));
	const int64_t nc = read_u32(w.number + nv, st);
	hipLaunchKernelGGL(k_simp_assign, grid(nv + 1), dim3(kThreads), 0, st, nv, nc, w.key2, w.vorder, w.head, w.number, sentinel, w.vcl, w.vfirst,
	                   w.ckey);
	FI_HIP_TRY(hipGetLastError());

	// primitives: the lowest of every oriented tuple of clusters, the clusters they use
	const int cbits = bits_for(nc);
	hipLaunchKernelGGL(k_simp_tuple_low<D>, grid(np), dim3(kThreads), 0, st, np, cbits, idx, w.vcl, w.tkey, w.tval);
	FI_HIP_TRY(hipGetLastError());
	sort_u64(w.tkey, w.tkey2, w.tval, w.tval2, np, 0, D == 3 ? 2 * cbits : cbits, w.tmp, st);
	hipLaunchKernelGGL(k_simp_tuple_high<D>, grid(np), dim3(kThreads), 0, st, np, w.tval2, idx, w.vcl, w.tkey);
	FI_HIP_TRY(hipGetLastError());
	sort_u64(w.tkey, w.tkey2, w.tval2, w.tval, np, 0, cbits, w.tmp, st);
	hipLaunchKernelGGL(k_simp_keep<D>, grid(np), dim3(kThreads), 0, st, np, w.tval, idx, w.vcl, w.keep);
	hipLaunchKernelGGL(k_simp_cluster_flags<D>, grid(np), dim3(kThreads), 0, st, np, w.keep, idx, w.vcl, w.cused);
	FI_HIP_TRY(hipGetLastError());
	scan_u32(w.keep, w.pto, np + 1, w.tmp, st);
	scan_u32(w.cused, w.cto, nc + 1, w.tmp, st);
	o->np = read_u32(w.pto + np, st);
	o->nv = read_u32(w.cto + nc, st);
	if (o->np == 0) {
		o->nv = 0;
		if (dmap) {
			hipLaunchKernelGGL(k_simp_vertex_map, grid(nv), dim3(kThreads), 0, st, nv, w.vcl, static_cast<const uint32_t*>(nullptr),
			                   static_cast<const uint32_t*>(nullptr), dmap);
		}
		FI_HIP_TRY(hipGetLastError());
		FI_HIP_TRY(hipStreamSynchronize(st));
		return;
	}

	// placement
	if (quadric) {
		const int64_t n = np * D;
		hipLaunchKernelGGL(k_simp_pairs<D>, grid(np), dim3(kThreads), 0, st, np, nc, idx, w.vcl, w.pkey, w.pval);
		FI_HIP_TRY(hipGetLastError());
		sort_u64(w.pkey, w.pkey2, w.pval, w.porder, n, 0, bits_for(nc + 1), w.tmp, st);
		hipLaunchKernelGGL(k_simp_pair_first, grid(n + 1), dim3(kThreads), 0, st, n, nc, w.pkey2, w.pfirst);
		FI_HIP_TRY(hipGetLastError());
	}
	PlaceArgs a{};
	a.nc     = nc;
	a.g      = g;
	a.cused  = w.cused;
	a.ckey   = w.ckey;
	a.vfirst = w.vfirst;
	a.vorder = w.vorder;
	a.pfirst = w.pfirst;
	a.porder = w.porder;
	a.idx    = idx;
	a.pos    = pos;
	a.nrm    = nrm;
	a.cpos   = w.cpos;
	a.cnrm   = w.cnrm;
	if (quadric) {
		hipLaunchKernelGGL((k_simp_place<D, true>), grid(nc), dim3(kThreads), 0, st, a);
	} else {
		hipLaunchKernelGGL((k_simp_place<D, false>), grid(nc), dim3(kThreads), 0, st, a);
	}
	FI_HIP_TRY(hipGetLastError());

	// gather
	o->pos.alloc(sizeof(float) * D * o->nv);
	if (nrm) { o->nrm.alloc(sizeof(float) * D * o->nv); }
	o->key.alloc(sizeof(int64_t) * o->nv);
	o->idx.alloc(sizeof(int) * D * o->np);
	hipLaunchKernelGGL(k_simp_gather_vertices<D>, grid(nc), dim3(kThreads), 0, st, nc, w.cused, w.cto, w.cpos, w.cnrm, w.ckey, o->pos.as<float>(),
	                   o->nrm.as<float>(), o->key.as<long long>());
	hipLaunchKernelGGL(k_simp_gather_prims<D>, grid(np), dim3(kThreads), 0, st, np, w.keep, w.pto, w.cto, idx, w.vcl, o->idx.as<int>());
	if (dmap) { hipLaunchKernelGGL(k_simp_vertex_map, grid(nv), dim3(kThreads), 0, st, nv, w.vcl, w.cused, w.cto, dmap); }
	FI_HIP_TRY(hipGetLastError());
	FI_HIP_TRY(hipStreamSynchronize(st));
}

}  // namespace

void mesh_simplify(const fi_mesh* m, float cell, const float* origin, int placement, int* vertex_map, int memory, fi_mesh** out)
{
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "out is null");
	*out = nullptr;
	FI_REQUIRE(m != nullptr, FI_ERR_INVALID, "null mesh");
	FI_REQUIRE(m->ndim == 2 || m->ndim == 3, FI_ERR_INVALID, "a mesh of %d-vertex primitives", m->ndim);
	check_memory(memory);
	FI_REQUIRE(cell > 0.0f, FI_ERR_INVALID, "cell must be > 0 (got %g)", static_cast<double>(cell));  // (false for a NaN)
	FI_REQUIRE(placement == FI_SIMPLIFY_QUADRIC || placement == FI_SIMPLIFY_MEAN, FI_ERR_INVALID, "bad placement %d", placement);
	FI_HIP_TRY(hipSetDevice(m->device));
	Grid g{};
	g.cell = cell;
	for (int d = 0; d < m->ndim; ++d) { g.o[d] = origin ? origin[d] : 0.0f; }
	std::unique_ptr<fi_mesh> o(new fi_mesh());
	o->device      = m->device;
	o->ndim        = m->ndim;
	o->has_normals = m->has_normals;
	hipStream_t st   = nullptr;
	stage::Out<int> dmap(m->nv > 0 ? vertex_map : nullptr, m->nv, memory);
	if (m->nv > 0 && m->np > 0) {
		if (m->ndim == 2) {
			simplify<2>(m, g, placement == FI_SIMPLIFY_QUADRIC, dmap, o.get(), st);
		} else {
			simplify<3>(m, g, placement == FI_SIMPLIFY_QUADRIC, dmap, o.get(), st);
		}
	} else if (dmap) {
		FI_HIP_TRY(hipMemsetAsync(dmap, 0xff, sizeof(int) * m->nv, st));
		FI_HIP_TRY(hipStreamSynchronize(st));
	}
	if (dmap.host) {  // (the work above has ended; this copy has its own wait)
		dmap.back(st);
		FI_HIP_TRY(hipStreamSynchronize(st));
	}
	*out = o.release();
}

}  // namespace fi
