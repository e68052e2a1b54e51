// fi_iso.h -- iso-contour / iso-surface extraction (fi_iso.hip), shared by the C ABI units (fi_capi.hip, fi_group.hip).
#pragma once

#include <memory>
#include <mutex>

#include "fi_internal.h"
#include "fi_prim.h"

namespace fi {
struct MeshParts;  // the labelling of a mesh's connected parts and what hangs on it (fi_parts.hip)
}

// the device-resident mesh of fi_iso_extract* / fi_dual_contour* / fi_mesh_create (include/fi_hip.h); immutable once built
struct fi_mesh {
	int        device = 0;
	int        ndim = 0;
	int64_t    nv = 0, np = 0;   // vertices, primitives (segments in 2-D, triangles in 3-D)
	fi::DevBuf pos, nrm;         // float[nv][ndim]
	fi::DevBuf idx;              // int32[np][ndim]
	fi::DevBuf key;              // int64[nv], ascending
	bool       has_normals = true;  // false: a caller's mesh without normals (fi_mesh_create): nrm is empty
	// the connected parts, computed at first use (fi_mesh_parts / fi_mesh_measure / fi_mesh_select) and kept with the handle
	mutable std::mutex                     parts_lock;
	mutable std::shared_ptr<fi::MeshParts> parts;
};

namespace fi {

// A whole field on the device (float, x fastest).  `pieces` meshes: piece r holds the cells whose slowest coordinate lies in
// the equal slab split's [lo_r, hi_r) (fi_slab_partition), with every vertex they use; pieces == 1: the undivided mesh.
void iso_extract_whole(const float* field, int ndim, const int* sizes, float iso, int pieces, const int* slab_lo,
                       const int* slab_hi, hipStream_t st, fi_mesh** out);
// The piece of a slab context (nranks > 1, its own transport) or the mesh of an undivided one.  field: the context's owned
// values (memory: FI_HOST / FI_DEVICE) or nullptr for the last solution.
void iso_extract_ctx(fi_ctx* c, const float* field, float iso, int memory, fi_mesh** out);
// a loop-back group's members, in rank order.  whole: the undivided field on the host (each piece reads its window of it),
// or nullptr: the members' last solutions, through the same ghost-plane exchange as iso_extract_ctx's slab contexts
void iso_extract_group(std::vector<fi_ctx*>& members, const float* whole, float iso, fi_mesh** out);

// ---- shared by the mesh extractors (fi_iso.hip, fi_dual.hip) ----------------------------------------------------------

// the lattice a mesh is extracted from: 2-D or 3-D (one_d: the extractor's message for a 1-D one), below 2^40 points
inline void check_mesh_dims(int ndim, const int* sizes, const char* one_d)
{
	FI_REQUIRE(sizes != nullptr, FI_ERR_INVALID, "sizes is null");
	FI_REQUIRE(ndim != 1, FI_ERR_UNSUPPORTED, "%s", one_d);
	FI_REQUIRE(ndim == 2 || ndim == 3, FI_ERR_INVALID, "ndim must be 2 or 3 (got %d)", ndim);
	int64_t n = 1;
	for (int d = 0; d < ndim; ++d) {
		FI_REQUIRE(sizes[d] >= 1, FI_ERR_INVALID, "sizes[%d] = %d", d, sizes[d]);
		n *= sizes[d];
	}
	FI_REQUIRE(n < (int64_t(1) << 40), FI_ERR_UNSUPPORTED, "lattice too large");
}

// exclusive prefix of x over a workgroup of THREADS; *total: the workgroup's sum (every thread)
template <int THREADS>
__device__ inline uint32_t block_scan(uint32_t x, uint32_t* total)
{
	__shared__ uint32_t s[THREADS / 64];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t inc = x;
	for (int o = 1; o < 64; o <<= 1) {
		const uint32_t y = __shfl_up(inc, o, 64);
		if (lane >= o) { inc += y; }
	}
	if (lane == 63) { s[wave] = inc; }
	__syncthreads();
	uint32_t pre = 0, all = 0;
	for (int w = 0; w < THREADS / 64; ++w) {
		pre += w < wave ? s[w] : 0u;
		all += s[w];
	}
	*total = all;
	return pre + inc - x;
}

// the scanned offsets an extractor's emit kernels start from: where work group b's vertices (sv[b]) and primitives (sp[b])
// begin, entry nb of each the total.  They live in `scan` and die with it.
struct ExtractScans {
	DevBuf          wg, scan, tot, tmp;
	const uint64_t *sv = nullptr, *sp = nullptr;
};

// The host sequence of an extractor up to its emit kernels, over nb work groups.  count(wg_v, wg_p, flag) launches the unit's
// count kernel (the groups' vertex and primitive counts, uint32[nb + 1] each with a trailing zero; the non-finite flag),
// totals(sv, sp, flag, tot) its totals kernel (tot: uint64[3] = vertices, primitives, flag).  Between them the two exclusive
// scans (rocPRIM); behind them the one read-back, the checks, m's sizes and its arrays.  False: the mesh is empty.
// (The four temporaries are allocations of their own, made where fi_iso.hip and fi_dual.hip made them before they shared this,
// the workspace behind the count kernel's launch.  With all of them made first, as one block or as four, the extraction took
// the same time but fi_mesh_copy of the finished mesh to the host took 1.7 ms instead of 0.65 and fi.iso_surface 25 ms instead
// of 16; why is not understood.  profiles/iso_surface.md has the variants and their figures.)
template <int D, class Count, class Totals>
bool extract_sizes(int64_t nb, hipStream_t st, fi_mesh* m, ExtractScans& s, Count&& count, Totals&& totals)
{
	FI_REQUIRE(nb < (int64_t(1) << 31), FI_ERR_UNSUPPORTED, "lattice too large");
	s.wg.alloc(sizeof(uint32_t) * (2 * (nb + 1) + 1));
	s.scan.alloc(sizeof(uint64_t) * 2 * (nb + 1));
	s.tot.alloc(sizeof(uint64_t) * 3);
	uint32_t* wg_v = s.wg.as<uint32_t>();
	uint32_t* wg_p = wg_v + (nb + 1);
	uint32_t* flag = wg_p + (nb + 1);
	uint64_t* sv   = s.scan.as<uint64_t>();
	uint64_t* sp   = sv + (nb + 1);
	uint64_t* tot  = s.tot.as<uint64_t>();
	FI_HIP_TRY(hipMemsetAsync(s.wg.p, 0, s.wg.bytes, st));  // (the trailing zero of each total list, the flag)
	count(wg_v, wg_p, flag);
	FI_HIP_TRY(hipGetLastError());
	s.tmp.alloc(prim::scan_bytes<uint64_t>(nb + 1));  // (here, behind the count kernel's launch: see above)
	const prim::Scratch tmp{s.tmp.p, s.tmp.bytes};
	prim::scan_u32(wg_v, sv, nb + 1, tmp, st);
	prim::scan_u32(wg_p, sp, nb + 1, tmp, st);
	totals(sv, sp, flag, tot);
	FI_HIP_TRY(hipGetLastError());
	uint64_t h[3] = {0, 0, 0};
	FI_HIP_TRY(hipMemcpyAsync(h, tot, sizeof(h), hipMemcpyDeviceToHost, st));
	FI_HIP_TRY(hipStreamSynchronize(st));
	FI_REQUIRE(h[2] == 0, FI_ERR_INVALID, "the field holds a non-finite value");
	FI_REQUIRE(h[0] < (uint64_t(1) << 31), FI_ERR_UNSUPPORTED, "the mesh would have %llu vertices (int32 indices)",
	           static_cast<unsigned long long>(h[0]));
	m->nv = static_cast<int64_t>(h[0]);
	m->np = static_cast<int64_t>(h[1]);
	if (m->nv == 0) { return false; }
	m->pos.alloc(sizeof(float) * D * m->nv);
	m->nrm.alloc(sizeof(float) * D * m->nv);
	m->key.alloc(sizeof(int64_t) * m->nv);
	m->idx.alloc(sizeof(int) * D * (m->np > 0 ? m->np : 1));
	s.sv = sv;
	s.sp = sp;
	return true;
}

}  // namespace fi
