// fi_parts.hip -- the connected parts of a device mesh: labels, per-part counts and measures, sub-meshes of chosen parts.
//
// The contract (include/fi_hip.h fi_mesh_create .. fi_mesh_select; tests/mesh_parts_reference.py is its
// definition in numpy): parts joined through shared vertex INDICES, numbered by their smallest vertex; exact integer counts
// of vertices, primitives, edges, boundary and irregular edges (2-D: vertices); fp64 size and enclosed measure summed in a
// fixed order; fp32 bounding boxes.  Nothing here depends on the run or the launch shape.
//
// How it is found:
//   labels    a union-find over the vertices, one 32-bit parent word each.  Every primitive finds the roots of its ends
//             (halving the paths it walks) and hooks the LARGER root under the smaller by a compare-and-swap on that root's
//             own word: a parent never exceeds its child, so the forest has no cycle and a part's root is its smallest
//             vertex whatever the timing.  A failed swap means another thread's swap on that word succeeded; the loser finds
//             again -- no thread waits for a value another workgroup has yet to write.  A second launch jumps every vertex
//             to its root (k_orient_jump's loop), root flags are scanned into dense numbers, and vertices and primitives
//             take their root's number.
//   counts    3-D: every half-edge as the 64-bit key min << 32 | max with its direction as the value, sorted (fi_prim.h's
//             Onesweep); the head of each run of equal keys classifies it by looking two entries ahead.  2-D: in- and
//             out-degrees by integer atomics.  Per-part totals by integer atomics, one per wave where its lanes agree.
//   measures  primitive numbers sorted by part (stable: ascending within a part); a workgroup per chunk of kChunk of a
//             part's primitives sums their terms by a fixed tree and reduces their bounding box; one thread per part adds
//             its chunks' partials in ascending order.  No floating-point atomics.
//   select    keep flags per vertex and primitive, exclusive scans, a gather with remapped indices.
#include "fi_solver_internal.h"
#include "fi_stage.h"
#include "fi_parts.h"
#include "fi_prim.h"
#include "fi_treesum.h"
#include "fi_unionfind.h"

#include <algorithm>
#include <memory>

namespace fi {

// what a mesh keeps of its parts (fi_mesh::parts)
struct MeshParts {
	int64_t                   count = 0;
	DevBuf                    vlabel, plabel;  // int32[nv], int32[np]
	bool                      measured = false;
	std::vector<fi_mesh_part> rows;
};

namespace {

using namespace unionfind;  // word_load, word_store, find_root, unite

constexpr int kChunk = treesum::kChunk;  // primitives a workgroup of the measuring pass sums: one each

// ---- labels ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_parts_start(int64_t nv, uint32_t* __restrict__ parent, uint32_t* __restrict__ used)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i > nv) { return; }
	used[i] = 0;  // (entry nv: the scans' total)
	if (i < nv) { parent[i] = static_cast<uint32_t>(i); }
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_parts_union(int64_t np, const int* __restrict__ idx, uint32_t* parent, uint32_t* __restrict__ used)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (p >= np) { return; }
	uint32_t v[D];
#pragma unroll
	for (int k = 0; k < D; ++k) {
		v[k]       = static_cast<uint32_t>(idx[p * D + k]);
		used[v[k]] = 1;
	}
#pragma unroll
	for (int k = 1; k < D; ++k) {
		if (v[k] != v[0]) { unite(parent, v[0], v[k]); }
	}
}

// every vertex straight under its root (roots do not move in this kernel)
__global__ __launch_bounds__(kThreads) void k_parts_jump(int64_t nv, uint32_t* parent)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= nv) { return; }
	for (;;) {
		const uint32_t p = word_load(&parent[i]);
		if (p == i) { break; }
		const uint32_t g = word_load(&parent[p]);
		if (g == p) { break; }
		word_store(&parent[i], g);
	}
}

__global__ __launch_bounds__(kThreads) void k_parts_roots(int64_t nv, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ used,
                                                           uint32_t* __restrict__ flag)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i > nv) { return; }
	flag[i] = i < nv && used[i] && parent[i] == i ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void k_parts_label_vertices(int64_t nv, const uint32_t* __restrict__ parent,
                                                                    const uint32_t* __restrict__ used, const uint32_t* __restrict__ number,
                                                                    int* __restrict__ vlabel)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= nv) { return; }
	vlabel[i] = used[i] ? static_cast<int>(number[parent[i]]) : -1;
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_parts_label_prims(int64_t np, const int* __restrict__ idx, const int* __restrict__ vlabel,
                                                                 int* __restrict__ plabel)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (p >= np) { return; }
	plabel[p] = vlabel[idx[p * D]];
}

// ---- caller meshes ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_parts_check(int64_t n, const int* __restrict__ idx, int64_t nv, uint32_t* __restrict__ bad)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	const int v = idx[i];
	if (v < 0 || v >= nv) { *bad = 1; }
}

__global__ __launch_bounds__(kThreads) void k_parts_iota(int64_t n, long long* __restrict__ out)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i < n) { out[i] = i; }
}

// ---- counts -----------------------------------------------------------------------------------------------------------

enum { kColVertices = 0, kColPrimitives = 1, kColEdges = 2, kColBoundary = 3, kColIrregular = 4, kCols = 5 };

// table[part][col] += 1 for the lanes that are `on`: one add per wave where they agree on the part.  Every lane of the wave
// calls this.
__device__ inline void part_add(unsigned long long* table, int col, int part, bool on)
{
	const unsigned long long m = __ballot(on);
	if (m == 0) { return; }
	const int  src   = __ffsll(m) - 1;
	const int  first = __shfl(part, src, 64);
	const bool split = __any(on && part != first);
	if (!split) {
		if ((threadIdx.x & 63) == src) { atomicAdd(&table[static_cast<int64_t>(first) * kCols + col], static_cast<unsigned long long>(__popcll(m))); }
	} else if (on) {
		atomicAdd(&table[static_cast<int64_t>(part) * kCols + col], 1ull);
	}
}

constexpr uint64_t kNoEdge = ~uint64_t(0);  // a half-edge with equal ends: sorted behind every other, never counted

__global__ __launch_bounds__(kThreads) void k_parts_halfedges(int64_t np, const int* __restrict__ idx, uint64_t* __restrict__ key,
                                                               uint8_t* __restrict__ dir)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (p >= np) { return; }
	uint32_t v[3];
#pragma unroll
	for (int k = 0; k < 3; ++k) { v[k] = static_cast<uint32_t>(idx[p * 3 + k]); }
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const uint32_t a = v[k], b = v[(k + 1) % 3];
		const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
		key[p * 3 + k] = a == b ? kNoEdge : (static_cast<uint64_t>(lo) << 32) | hi;
		dir[p * 3 + k] = a < b ? 0 : 1;
	}
}

// the sorted half-edges: the first of a run of equal keys is the edge, and says what kind
__global__ __launch_bounds__(kThreads) void k_parts_classify(int64_t n, const uint64_t* __restrict__ key, const uint8_t* __restrict__ dir,
                                                              const int* __restrict__ vlabel, unsigned long long* table)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	bool          head = false, boundary = false, irregular = false;
	int           part = 0;
	if (i < n) {
		const uint64_t k = key[i];
		head = k != kNoEdge && (i == 0 || key[i - 1] != k);
		if (head) {
			part = vlabel[k >> 32];
			const bool two   = i + 1 < n && key[i + 1] == k;
			const bool three = two && i + 2 < n && key[i + 2] == k;
			boundary  = !two;
			irregular = three || (two && dir[i] == dir[i + 1]);
		}
	}
	part_add(table, kColEdges, part, head);
	part_add(table, kColBoundary, part, boundary);
	part_add(table, kColIrregular, part, irregular);
}

// 2-D: a segment (a, b), a != b, leaves a and enters b
__global__ __launch_bounds__(kThreads) void k_parts_degrees(int64_t np, const int* __restrict__ idx, const int* __restrict__ plabel,
                                                             uint32_t* deg_in, uint32_t* deg_out, unsigned long long* table)
{
	const int64_t p    = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	bool          edge = false;
	int           part = 0;
	if (p < np) {
		const int a = idx[2 * p], b = idx[2 * p + 1];
		part = plabel[p];
		edge = a != b;
		if (edge) {
			atomicAdd(&deg_out[a], 1u);
			atomicAdd(&deg_in[b], 1u);
		}
	}
	part_add(table, kColEdges, part, edge);
}

__global__ __launch_bounds__(kThreads) void k_parts_count_prims(int64_t np, const int* __restrict__ plabel, unsigned long long* table)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	part_add(table, kColPrimitives, p < np ? plabel[p] : 0, p < np);
}

// the part's vertices; 2-D (deg_in != nullptr): its ends and its irregular vertices too
__global__ __launch_bounds__(kThreads) void k_parts_count_vertices(int64_t nv, const int* __restrict__ vlabel, const uint32_t* __restrict__ deg_in,
                                                                    const uint32_t* __restrict__ deg_out, unsigned long long* table)
{
	const int64_t i    = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	const int     part = i < nv ? vlabel[i] : -1;
	const bool    on   = part >= 0;
	part_add(table, kColVertices, part, on);
	if (deg_in == nullptr) { return; }
	bool end = false, odd = false;
	if (on) {
		const uint32_t in = deg_in[i], out = deg_out[i];
		end = in + out == 1;
		odd = !end && !(in == 1 && out == 1);
	}
	part_add(table, kColBoundary, part, end);
	part_add(table, kColIrregular, part, odd);
}

// ---- measures ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_parts_sort_keys(int64_t np, const int* __restrict__ plabel, uint64_t* __restrict__ key,
                                                               uint32_t* __restrict__ val)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (p >= np) { return; }
	key[p] = static_cast<uint64_t>(plabel[p]);
	val[p] = static_cast<uint32_t>(p);
}

// first[c]: where part c begins in the sorted list (every part has a primitive); first[C] = np
__global__ __launch_bounds__(kThreads) void k_parts_first(int64_t np, int64_t nparts, const uint64_t* __restrict__ key, uint32_t* __restrict__ first)
{
	const int64_t s = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (s > np) { return; }
	if (s == np) {
		first[nparts] = static_cast<uint32_t>(np);
	} else if (s == 0 || key[s - 1] != key[s]) {
		first[key[s]] = static_cast<uint32_t>(s);
	}
}

__global__ __launch_bounds__(kThreads) void k_parts_chunk_counts(int64_t nparts, const uint32_t* __restrict__ first, uint32_t* __restrict__ nchunks)
{
	const int64_t c = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (c > nparts) { return; }
	nchunks[c] = treesum::chunks_of(first, c, nparts);
}

struct ChunkPartial {
	double size, enclosed;
	float  lo[3], hi[3];
};

__device__ inline float wave_min(float v)
{
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1) { v = fminf(v, __shfl_xor(v, o, 64)); }
	return v;
}
__device__ inline float wave_max(float v)
{
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1) { v = fmaxf(v, __shfl_xor(v, o, 64)); }
	return v;
}

// one workgroup per chunk: chunk j of part c holds the part's sorted primitives [kChunk j, kChunk (j + 1)), one a thread.
// The terms are summed by wave_sum's tree within each wave (lane 0 holds the sum) and the four waves' sums added in wave order.
template <int D>
__global__ __launch_bounds__(kChunk) void k_parts_chunks(int64_t nparts, const uint32_t* __restrict__ first, const uint32_t* __restrict__ chunk_first,
                                                          const uint32_t* __restrict__ order, const int* __restrict__ idx,
                                                          const float* __restrict__ pos, ChunkPartial* __restrict__ out)
{
	__shared__ double s_sum[2][kChunk / 64];
	__shared__ float  s_box[6][kChunk / 64];
	const uint32_t chunk = blockIdx.x;
	const int64_t  lo    = treesum::owner_of(chunk_first, nparts, chunk);  // the part of this chunk (every part has one)
	const uint32_t begin = first[lo] + (chunk - chunk_first[lo]) * kChunk, end = first[lo + 1];
	const uint32_t s     = begin + threadIdx.x;
	double         size = 0.0, enclosed = 0.0;
	float          bl[3] = {INFINITY, INFINITY, INFINITY}, bh[3] = {-INFINITY, -INFINITY, -INFINITY};
	if (s < end) {
		const int64_t p = order[s];
		double        x[D][D];
#pragma unroll
		for (int k = 0; k < D; ++k) {
			const int64_t v = idx[p * D + k];
#pragma unroll
			for (int d = 0; d < D; ++d) {
				const float f = pos[v * D + d];
				x[k][d] = static_cast<double>(f);
				bl[d]   = fminf(bl[d], f);
				bh[d]   = fmaxf(bh[d], f);
			}
		}
		if constexpr (D == 3) {
			double u[3], w[3];
#pragma unroll
			for (int d = 0; d < 3; ++d) {
				u[d] = x[1][d] - x[0][d];
				w[d] = x[2][d] - x[0][d];
			}
			const double nx = u[1] * w[2] - u[2] * w[1], ny = u[2] * w[0] - u[0] * w[2], nz = u[0] * w[1] - u[1] * w[0];
			size = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
			const double* a = x[0];
			const double* b = x[1];
			const double* c = x[2];
			const double  cx = b[1] * c[2] - b[2] * c[1], cy = b[2] * c[0] - b[0] * c[2], cz = b[0] * c[1] - b[1] * c[0];
			enclosed = ((a[0] * cx + a[1] * cy) + a[2] * cz) / 6.0;
		} else {
			const double dx = x[1][0] - x[0][0], dy = x[1][1] - x[0][1];
			size     = sqrt(dx * dx + dy * dy);
			enclosed = 0.5 * (x[0][0] * x[1][1] - x[0][1] * x[1][0]);
		}
	}
	const int wave = threadIdx.x >> 6;
	size     = wave_sum(size);
	enclosed = wave_sum(enclosed);
#pragma unroll
	for (int d = 0; d < D; ++d) {
		bl[d] = wave_min(bl[d]);
		bh[d] = wave_max(bh[d]);
	}
	if ((threadIdx.x & 63) == 0) {
		s_sum[0][wave] = size;
		s_sum[1][wave] = enclosed;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			s_box[d][wave]     = bl[d];
			s_box[3 + d][wave] = bh[d];
		}
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		ChunkPartial r{};
		for (int w = 0; w < kChunk / 64; ++w) {
			r.size     = r.size + s_sum[0][w];
			r.enclosed = r.enclosed + s_sum[1][w];
		}
		for (int d = 0; d < 3; ++d) {
			r.lo[d] = r.hi[d] = 0.0f;
			if (d < D) {
				r.lo[d] = s_box[d][0];
				r.hi[d] = s_box[3 + d][0];
				for (int w = 1; w < kChunk / 64; ++w) {
					r.lo[d] = fminf(r.lo[d], s_box[d][w]);
					r.hi[d] = fmaxf(r.hi[d], s_box[3 + d][w]);
				}
			}
		}
		out[chunk] = r;
	}
}

// one thread per part: its chunks in ascending order, and its row
__global__ __launch_bounds__(kThreads) void k_parts_rows(int64_t nparts, const uint32_t* __restrict__ chunk_first, const ChunkPartial* __restrict__ partial,
                                                          const unsigned long long* __restrict__ table, fi_mesh_part* __restrict__ rows)
{
	const int64_t c = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (c >= nparts) { return; }
	const uint32_t b = chunk_first[c], e = chunk_first[c + 1];
	ChunkPartial   r = partial[b];
	for (uint32_t k = b + 1; k < e; ++k) {
		const ChunkPartial q = partial[k];
		r.size     = r.size + q.size;
		r.enclosed = r.enclosed + q.enclosed;
		for (int d = 0; d < 3; ++d) {
			r.lo[d] = fminf(r.lo[d], q.lo[d]);
			r.hi[d] = fmaxf(r.hi[d], q.hi[d]);
		}
	}
	fi_mesh_part o;
	o.vertices   = static_cast<long long>(table[c * kCols + kColVertices]);
	o.primitives = static_cast<long long>(table[c * kCols + kColPrimitives]);
	o.edges      = static_cast<long long>(table[c * kCols + kColEdges]);
	o.boundary   = static_cast<long long>(table[c * kCols + kColBoundary]);
	o.irregular  = static_cast<long long>(table[c * kCols + kColIrregular]);
	o.size       = r.size;
	o.enclosed   = r.enclosed;
	for (int d = 0; d < 3; ++d) {
		o.lo[d] = r.lo[d];
		o.hi[d] = r.hi[d];
	}
	rows[c] = o;
}

// ---- select -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_parts_keep_flags(int64_t n, const int* __restrict__ label, const uint8_t* __restrict__ keep,
                                                                uint32_t* __restrict__ flag)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i > n) { return; }
	uint32_t f = 0;
	if (i < n) {
		const int c = label[i];
		f = c >= 0 && keep[c] ? 1u : 0u;
	}
	flag[i] = f;  // (entry n: the scan's total)
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_parts_gather_vertices(int64_t nv, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ to,
                                                                     const float* __restrict__ pos, const float* __restrict__ nrm,
                                                                     const long long* __restrict__ key, float* __restrict__ pos_out,
                                                                     float* __restrict__ nrm_out, long long* __restrict__ key_out)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= nv || !flag[i]) { return; }
	const int64_t j = to[i];
#pragma unroll
	for (int d = 0; d < D; ++d) {
		pos_out[j * D + d] = pos[i * D + d];
		if (nrm) { nrm_out[j * D + d] = nrm[i * D + d]; }
	}
	key_out[j] = key[i];
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_parts_gather_prims(int64_t np, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ to,
                                                                  const uint32_t* __restrict__ vertex_to, const int* __restrict__ idx,
                                                                  int* __restrict__ idx_out)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (p >= np || !flag[p]) { return; }
	const int64_t q = to[p];
#pragma unroll
	for (int k = 0; k < D; ++k) { idx_out[q * D + k] = static_cast<int>(vertex_to[idx[p * D + k]]); }
}

// ---- host side --------------------------------------------------------------------------------------------------------

using namespace prim;  // Arena, Scratch, scan_u32, sort_u64, read_u32, bits_for, grid
static_assert(kThreads == kGridThreads, "grid() counts work groups of kThreads");

// Each call lays its temporaries out in one block (fi_arena.h), the zeroed ones first, the primitives' workspace last.

template <int D>
void label(const fi_mesh* m, MeshParts* P, hipStream_t st)
{
	const int64_t nv = m->nv, np = m->np;
	P->vlabel.alloc(sizeof(int) * (nv > 0 ? nv : 1));
	P->plabel.alloc(sizeof(int) * (np > 0 ? np : 1));
	P->count = 0;
	if (nv == 0) { return; }
	uint32_t *parent = nullptr, *used = nullptr, *flag = nullptr, *number = nullptr;
	Scratch   tmp;
	tmp.bytes = scan_bytes(nv + 1);
	DevBuf block;
	arena_alloc(block, [&](Arena& a) {
		parent = a.take<uint32_t>(nv);
		used   = a.take<uint32_t>(nv + 1);
		flag   = a.take<uint32_t>(nv + 1);
		number = a.take<uint32_t>(nv + 1);
		tmp.p  = a.take<char>(static_cast<int64_t>(tmp.bytes));
	});
	hipLaunchKernelGGL(k_parts_start, grid(nv + 1), dim3(kThreads), 0, st, nv, parent, used);
	if (np > 0) { hipLaunchKernelGGL(k_parts_union<D>, grid(np), dim3(kThreads), 0, st, np, m->idx.as<int>(), parent, used); }
	hipLaunchKernelGGL(k_parts_jump, grid(nv), dim3(kThreads), 0, st, nv, parent);
	hipLaunchKernelGGL(k_parts_roots, grid(nv + 1), dim3(kThreads), 0, st, nv, parent, used, flag);
	FI_HIP_TRY(hipGetLastError());
	scan_u32(flag, number, nv + 1, tmp, st);
	hipLaunchKernelGGL(k_parts_label_vertices, grid(nv), dim3(kThreads), 0, st, nv, parent, used, number, P->vlabel.as<int>());
	if (np > 0) {
		hipLaunchKernelGGL(k_parts_label_prims<D>, grid(np), dim3(kThreads), 0, st, np, m->idx.as<int>(), P->vlabel.as<int>(), P->plabel.as<int>());
	}
	FI_HIP_TRY(hipGetLastError());
	P->count = read_u32(number + nv, st);  // (synchronises: the temporaries die here)
}

template <int D>
void measure(const fi_mesh* m, MeshParts* P, hipStream_t st)
{
	const int64_t nv = m->nv, np = m->np, C = P->count;
	P->rows.assign(static_cast<size_t>(C), fi_mesh_part{});
	if (C == 0) {
		P->measured = true;
		return;
	}
	const int*    vlabel = P->vlabel.as<int>();
	const int*    plabel = P->plabel.as<int>();
	const int*    idx    = m->idx.as<int>();
	const int64_t ne     = D == 3 ? 3 * np : 0;  // half-edges
	FI_REQUIRE(ne < (int64_t(1) << 32), FI_ERR_UNSUPPORTED, "the mesh has %lld half-edges", static_cast<long long>(ne));

	unsigned long long* T = nullptr;  // the counter table
	uint32_t *          deg = nullptr, *order0 = nullptr, *order = nullptr, *first = nullptr, *nchunks = nullptr, *chunk_first = nullptr;
	uint64_t *          key = nullptr, *key2 = nullptr, *skey = nullptr, *skey2 = nullptr;
	uint8_t *           dir = nullptr, *dir2 = nullptr;
	fi_mesh_part*       rows   = nullptr;
	size_t              zeroed = 0;
	Scratch             tmp;
	tmp.bytes = std::max(sort_bytes(np, 0, bits_for(C)), scan_bytes(C + 1));
	if (D == 3) { tmp.bytes = std::max(tmp.bytes, sort_bytes<uint8_t>(ne, 0, 64)); }
	DevBuf block;
	arena_alloc(block, [&](Arena& a) {
		T      = a.take<unsigned long long>(kCols * C);
		deg    = D == 2 ? a.take<uint32_t>(2 * nv) : nullptr;
		zeroed = a.bytes();
		if (D == 3) {
			key  = a.take<uint64_t>(ne);
			key2 = a.take<uint64_t>(ne);
			dir  = a.take<uint8_t>(ne);
			dir2 = a.take<uint8_t>(ne);
		}
		skey        = a.take<uint64_t>(np);
		skey2       = a.take<uint64_t>(np);
		order0      = a.take<uint32_t>(np);
		order       = a.take<uint32_t>(np);
		first       = a.take<uint32_t>(C + 1);
		nchunks     = a.take<uint32_t>(C + 1);
		chunk_first = a.take<uint32_t>(C + 1);
		rows        = a.take<fi_mesh_part>(C);
		tmp.p       = a.take<char>(static_cast<int64_t>(tmp.bytes));
	});
	FI_HIP_TRY(hipMemsetAsync(block.p, 0, zeroed, st));

	// the counts
	hipLaunchKernelGGL(k_parts_count_prims, grid(np), dim3(kThreads), 0, st, np, plabel, T);
	if (D == 3) {
		hipLaunchKernelGGL(k_parts_halfedges, grid(np), dim3(kThreads), 0, st, np, idx, key, dir);
		FI_HIP_TRY(hipGetLastError());
		sort_u64(key, key2, dir, dir2, ne, 0, 64, tmp, st);
		hipLaunchKernelGGL(k_parts_classify, grid(ne), dim3(kThreads), 0, st, ne, key2, dir2, vlabel, T);
		hipLaunchKernelGGL(k_parts_count_vertices, grid(nv), dim3(kThreads), 0, st, nv, vlabel, static_cast<const uint32_t*>(nullptr),
		                   static_cast<const uint32_t*>(nullptr), T);
	} else {
		uint32_t* din  = deg;
		uint32_t* dout = din + nv;
		hipLaunchKernelGGL(k_parts_degrees, grid(np), dim3(kThreads), 0, st, np, idx, plabel, din, dout, T);
		hipLaunchKernelGGL(k_parts_count_vertices, grid(nv), dim3(kThreads), 0, st, nv, vlabel, static_cast<const uint32_t*>(din),
		                   static_cast<const uint32_t*>(dout), T);
	}
	FI_HIP_TRY(hipGetLastError());

	// the measures: primitive numbers by part, chunks of a part, a part's chunks in order
	hipLaunchKernelGGL(k_parts_sort_keys, grid(np), dim3(kThreads), 0, st, np, plabel, skey, order0);
	FI_HIP_TRY(hipGetLastError());
	sort_u64(skey, skey2, order0, order, np, 0, bits_for(C), tmp, st);
	hipLaunchKernelGGL(k_parts_first, grid(np + 1), dim3(kThreads), 0, st, np, C, skey2, first);
	hipLaunchKernelGGL(k_parts_chunk_counts, grid(C + 1), dim3(kThreads), 0, st, C, first, nchunks);
	FI_HIP_TRY(hipGetLastError());
	scan_u32(nchunks, chunk_first, C + 1, tmp, st);
	const uint32_t total = read_u32(chunk_first + C, st);
	DevBuf         partial;  // (its size is known only now)
	partial.alloc(sizeof(ChunkPartial) * total);
	hipLaunchKernelGGL(k_parts_chunks<D>, dim3(total), dim3(kChunk), 0, st, C, first, chunk_first, order, idx, m->pos.as<float>(),
	                   partial.as<ChunkPartial>());
	hipLaunchKernelGGL(k_parts_rows, grid(C), dim3(kThreads), 0, st, C, chunk_first, partial.as<ChunkPartial>(), T, rows);
	FI_HIP_TRY(hipGetLastError());
	FI_HIP_TRY(hipMemcpyAsync(P->rows.data(), rows, sizeof(fi_mesh_part) * C, hipMemcpyDeviceToHost, st));
	FI_HIP_TRY(hipStreamSynchronize(st));
	P->measured = true;
}

// the mesh's labelling, computed at first use (the caller holds m->parts_lock)
MeshParts* ensure_labels(const fi_mesh* m)
{
	if (!m->parts) {
		auto P = std::make_shared<MeshParts>();
		if (m->ndim == 2) {
			label<2>(m, P.get(), nullptr);
		} else {
			label<3>(m, P.get(), nullptr);
		}
		m->parts = P;
	}
	return m->parts.get();
}

void check_mesh(const fi_mesh* m)
{
	FI_REQUIRE(m != nullptr, FI_ERR_INVALID, "null mesh");
	FI_REQUIRE(m->ndim == 2 || m->ndim == 3, FI_ERR_INVALID, "a mesh of %d-vertex primitives", m->ndim);
	FI_HIP_TRY(hipSetDevice(m->device));
}

template <int D>
void select(const fi_mesh* m, const MeshParts* P, const uint8_t* keep, fi_mesh* o, hipStream_t st)
{
	const int64_t nv = m->nv, np = m->np;
	uint32_t *vflag = nullptr, *pflag = nullptr, *vto = nullptr, *pto = nullptr;
	Scratch   tmp;
	tmp.bytes = scan_bytes(std::max(nv, np) + 1);
	DevBuf block;
	arena_alloc(block, [&](Arena& a) {
		vflag = a.take<uint32_t>(nv + 1);
		pflag = a.take<uint32_t>(np + 1);
		vto   = a.take<uint32_t>(nv + 1);
		pto   = a.take<uint32_t>(np + 1);
		tmp.p = a.take<char>(static_cast<int64_t>(tmp.bytes));
	});
	hipLaunchKernelGGL(k_parts_keep_flags, grid(nv + 1), dim3(kThreads), 0, st, nv, P->vlabel.as<int>(), keep, vflag);
	hipLaunchKernelGGL(k_parts_keep_flags, grid(np + 1), dim3(kThreads), 0, st, np, P->plabel.as<int>(), keep, pflag);
	FI_HIP_TRY(hipGetLastError());
	scan_u32(vflag, vto, nv + 1, tmp, st);
	scan_u32(pflag, pto, np + 1, tmp, st);
	o->nv = read_u32(vto + nv, st);
	o->np = read_u32(pto + np, st);
	if (o->nv == 0) { return; }
	o->pos.alloc(sizeof(float) * D * o->nv);
	if (m->has_normals) { o->nrm.alloc(sizeof(float) * D * o->nv); }
	o->key.alloc(sizeof(int64_t) * o->nv);
	o->idx.alloc(sizeof(int) * D * (o->np > 0 ? o->np : 1));
	hipLaunchKernelGGL(k_parts_gather_vertices<D>, grid(nv), dim3(kThreads), 0, st, nv, vflag, vto, m->pos.as<float>(),
	                   m->has_normals ? m->nrm.as<float>() : nullptr, m->key.as<long long>(), o->pos.as<float>(), o->nrm.as<float>(),
	                   o->key.as<long long>());
	if (np > 0) {
		hipLaunchKernelGGL(k_parts_gather_prims<D>, grid(np), dim3(kThreads), 0, st, np, pflag, pto, vto, m->idx.as<int>(), o->idx.as<int>());
	}
	FI_HIP_TRY(hipGetLastError());
	FI_HIP_TRY(hipStreamSynchronize(st));
}

}  // namespace

void mesh_create(fi_mesh** out, int ndim, long num_vertices, const float* vertices, const float* normals, const long long* keys,
                 long num_primitives, const int* indices, int memory)
{
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "out is null");
	*out = nullptr;
	check_memory(memory);
	FI_REQUIRE(ndim == 2 || ndim == 3, FI_ERR_UNSUPPORTED, "a mesh has 2 or 3 dimensions (got %d)", ndim);
	FI_REQUIRE(num_vertices >= 0 && num_primitives >= 0, FI_ERR_INVALID, "negative count");
	FI_REQUIRE(num_vertices < (1LL << 31) && num_primitives < (1LL << 31), FI_ERR_UNSUPPORTED,
	           "%ld vertices, %ld primitives: int32 indices and labels", num_vertices, num_primitives);
	FI_REQUIRE(num_vertices == 0 || vertices != nullptr, FI_ERR_INVALID, "vertices is null");
	FI_REQUIRE(num_primitives == 0 || indices != nullptr, FI_ERR_INVALID, "indices is null");
	const int64_t nv = num_vertices, np = num_primitives;
	const size_t  D = static_cast<size_t>(ndim);
	std::unique_ptr<fi_mesh> m(new fi_mesh());
	FI_HIP_TRY(hipGetDevice(&m->device));
	m->ndim        = ndim;
	m->nv          = nv;
	m->np          = np;
	m->has_normals = normals != nullptr || nv == 0;
	const hipMemcpyKind kind = memory == FI_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
	hipStream_t         st   = nullptr;
	if (np > 0) {
		m->idx.alloc(sizeof(int) * D * np);
		FI_HIP_TRY(hipMemcpyAsync(m->idx.p, indices, sizeof(int) * D * np, kind, st));
		DevBuf bad;
		bad.alloc(sizeof(uint32_t));
		FI_HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(uint32_t), st));
		hipLaunchKernelGGL(k_parts_check, grid(np * ndim), dim3(kThreads), 0, st, np * ndim, m->idx.as<int>(), nv, bad.as<uint32_t>());
		FI_HIP_TRY(hipGetLastError());
		FI_REQUIRE(read_u32(bad.as<uint32_t>(), st) == 0, FI_ERR_INVALID, "an index lies outside [0, %ld)", num_vertices);
	}
	if (nv > 0) {
		m->pos.alloc(sizeof(float) * D * nv);
		FI_HIP_TRY(hipMemcpyAsync(m->pos.p, vertices, sizeof(float) * D * nv, kind, st));
		if (normals) {
			m->nrm.alloc(sizeof(float) * D * nv);
			FI_HIP_TRY(hipMemcpyAsync(m->nrm.p, normals, sizeof(float) * D * nv, kind, st));
		}
		m->key.alloc(sizeof(int64_t) * nv);
		if (keys) {
			FI_HIP_TRY(hipMemcpyAsync(m->key.p, keys, sizeof(int64_t) * nv, kind, st));
		} else {
			hipLaunchKernelGGL(k_parts_iota, grid(nv), dim3(kThreads), 0, st, nv, m->key.as<long long>());
			FI_HIP_TRY(hipGetLastError());
		}
	}
	FI_HIP_TRY(hipStreamSynchronize(st));
	*out = m.release();
}

void mesh_parts(const fi_mesh* m, long* num_parts, int* vertex_labels, int* primitive_labels, int memory)
{
	check_mesh(m);
	check_memory(memory);
	std::lock_guard<std::mutex> hold(m->parts_lock);
	const MeshParts*            P = ensure_labels(m);
	if (num_parts) { *num_parts = static_cast<long>(P->count); }
	const hipMemcpyKind kind = memory == FI_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
	if (vertex_labels && m->nv > 0) { FI_HIP_TRY(hipMemcpy(vertex_labels, P->vlabel.p, sizeof(int) * m->nv, kind)); }
	if (primitive_labels && m->np > 0) { FI_HIP_TRY(hipMemcpy(primitive_labels, P->plabel.p, sizeof(int) * m->np, kind)); }
}

void mesh_measure(const fi_mesh* m, long capacity, fi_mesh_part* parts, long* num_parts)
{
	check_mesh(m);
	std::lock_guard<std::mutex> hold(m->parts_lock);
	MeshParts*                  P = ensure_labels(m);
	if (num_parts) { *num_parts = static_cast<long>(P->count); }
	FI_REQUIRE(capacity >= P->count, FI_ERR_INVALID, "room for %ld parts, the mesh has %lld", capacity, static_cast<long long>(P->count));
	FI_REQUIRE(parts != nullptr || P->count == 0, FI_ERR_INVALID, "parts is null");
	if (!P->measured) {
		if (m->ndim == 2) {
			measure<2>(m, P, nullptr);
		} else {
			measure<3>(m, P, nullptr);
		}
	}
	for (int64_t c = 0; c < P->count; ++c) { parts[c] = P->rows[static_cast<size_t>(c)]; }
}

void mesh_select(const fi_mesh* m, long num_parts, const unsigned char* keep, fi_mesh** out)
{
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "out is null");
	*out = nullptr;
	check_mesh(m);
	std::lock_guard<std::mutex> hold(m->parts_lock);
	const MeshParts*            P = ensure_labels(m);
	FI_REQUIRE(num_parts == P->count, FI_ERR_INVALID, "keep has %ld entries, the mesh has %lld parts", num_parts,
	           static_cast<long long>(P->count));
	FI_REQUIRE(keep != nullptr || num_parts == 0, FI_ERR_INVALID, "keep is null");
	std::unique_ptr<fi_mesh> o(new fi_mesh());
	o->device      = m->device;
	o->ndim        = m->ndim;
	o->has_normals = m->has_normals;
	if (P->count > 0) {
		DevBuf dk;
		dk.alloc(static_cast<size_t>(num_parts));
		FI_HIP_TRY(hipMemcpy(dk.p, keep, static_cast<size_t>(num_parts), hipMemcpyHostToDevice));
		if (m->ndim == 2) {
			select<2>(m, P, dk.as<uint8_t>(), o.get(), nullptr);
		} else {
			select<3>(m, P, dk.as<uint8_t>(), o.get(), nullptr);
		}
	}
	*out = o.release();
}

}  // namespace fi
