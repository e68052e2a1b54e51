// fi_iso.hip -- iso-contours (2-D, marching squares) and iso-surfaces (3-D, marching cubes) of a lattice field, on the device.
//
// The contract ("Iso-contours and iso-surfaces"): inside is f < iso; one vertex per lattice edge whose ends
// differ in inside-ness, keyed ndim * index(p) + axis and stored in key order; primitives cell by cell in ascending linear
// index, each cell's taken from fi_iso_tables.h (tools/gen_iso_tables.py).  Three passes over the points of the planes a
// piece covers, one thread per point:
//   k_iso_count     crossing edges the point owns (0 .. ndim) and the primitives of the cell it is the lower corner of,
//                   summed per workgroup; the non-finite flag
//   (scan)          exclusive sums of the workgroup totals (rocPRIM); the two grand totals and the flag read back once
//   k_iso_vertices  the point's vertices at its scanned offset (positions, normals, keys) and its vertex base (uint32)
//   k_iso_prims     the cell's primitives at its scanned offset, vertex indices gathered from the bases of its corners
// Scratch: 4 bytes per point (the bases) plus the workgroup totals.
#include "fi_solver_internal.h"
#include "fi_stage.h"
#include "fi_prim.h"
#include "fi_iso.h"
#include "fi_iso_tables.h"

namespace fi {

namespace {

constexpr int kIsoThreads = 256;

// the planes of the slowest axis a launch sees: the window [wlo, whi) of the field (x fastest, starting at plane wlo);
// cells of slow coordinate [clo, chi), vertices on planes [clo, chi] (plane chi: only the edges inside the plane)
struct IsoView {
	const float* f;
	int     n[3];     // global extents (1 beyond ndim)
	int     wlo, whi;
	int     clo, chi;
	float   iso;
	int64_t plane;    // points per plane of the slowest axis
	int64_t npts;     // points of planes [clo, chi]
};

template <int D>
__device__ inline float ld(const IsoView& v, const int* c)
{
	int64_t i = c[0];
	if (D == 2) {
		i += static_cast<int64_t>(v.n[0]) * (c[1] - v.wlo);
	} else {
		i += static_cast<int64_t>(v.n[0]) * (c[1] + static_cast<int64_t>(v.n[1]) * (c[2] - v.wlo));
	}
	return v.f[i];
}

template <int D>
__device__ inline void coords(const IsoView& v, int64_t i, int* c)
{
	const int64_t s = i / v.plane;
	int64_t r = i - s * v.plane;
	c[D - 1] = v.clo + static_cast<int>(s);
	if (D == 3) {
		c[1] = static_cast<int>(r / v.n[0]);
		r -= static_cast<int64_t>(c[1]) * v.n[0];
	}
	c[0] = static_cast<int>(r);
}

// the edge (c, c + e_a) exists in this piece
template <int D>
__device__ inline bool edge_ok(const IsoView& v, const int* c, int a)
{
	return c[a] + 1 < v.n[a] && (a != D - 1 || c[a] < v.chi);
}

// bit a: the edge (c, c + e_a) crosses the iso value; *bad: a non-finite value among those read
template <int D>
__device__ inline unsigned crossings(const IsoView& v, const int* c, float fc, bool* bad)
{
	const bool in = fc < v.iso;
	unsigned m = 0;
	for (int a = 0; a < D; ++a) {
		if (!edge_ok<D>(v, c, a)) { continue; }
		int q[3] = {c[0], c[1], c[2]};
		q[a] += 1;
		const float fq = ld<D>(v, q);
		*bad = *bad || !isfinite(fq);
		if ((fq < v.iso) != in) { m |= 1u << a; }
	}
	return m;
}

template <int D>
__device__ inline bool is_cell(const IsoView& v, const int* c)
{
	for (int a = 0; a < D; ++a) {
		if (c[a] + 1 >= v.n[a]) { return false; }
	}
	return c[D - 1] < v.chi;
}

template <int D>
__device__ inline unsigned cell_case(const IsoView& v, const int* c)
{
	unsigned cs = 0;
	for (int k = 0; k < (1 << D); ++k) {
		int q[3] = {c[0] + (k & 1), c[1] + ((k >> 1) & 1), D == 3 ? c[2] + ((k >> 2) & 1) : 0};
		if (ld<D>(v, q) < v.iso) { cs |= 1u << k; }
	}
	return cs;
}

template <int D>
__device__ inline unsigned prims_of(unsigned cs)
{
	return D == 2 ? iso::kSqCount[cs] : iso::kCubeCount[cs];
}

template <int D>
__global__ __launch_bounds__(kIsoThreads) void k_iso_count(IsoView v, uint32_t* __restrict__ wg_v, uint32_t* __restrict__ wg_p,
                                                           uint32_t* __restrict__ flag)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kIsoThreads + threadIdx.x;
	uint32_t nv = 0, np = 0;
	bool bad = false;
	if (i < v.npts) {
		int c[3] = {0, 0, 0};
		coords<D>(v, i, c);
		const float fc = ld<D>(v, c);
		bad = !isfinite(fc);
		nv = __popc(crossings<D>(v, c, fc, &bad));
		if (is_cell<D>(v, c)) { np = prims_of<D>(cell_case<D>(v, c)); }
		// the planes next to [clo, chi] that only the normals read
		int q[3] = {c[0], c[1], c[2]};
		if (c[D - 1] == v.clo && v.clo > v.wlo) {
			q[D - 1] = v.clo - 1;
			bad = bad || !isfinite(ld<D>(v, q));
		}
		if (c[D - 1] == v.chi && v.chi + 1 < v.whi) {
			q[D - 1] = v.chi + 1;
			bad = bad || !isfinite(ld<D>(v, q));
		}
	}
	if (__any(bad) && (threadIdx.x & 63) == 0) { atomicOr(flag, 1u); }
	uint32_t tv = 0, tp = 0;
	(void)block_scan<kIsoThreads>(nv, &tv);
	__syncthreads();
	(void)block_scan<kIsoThreads>(np, &tp);
	if (threadIdx.x == 0) {
		wg_v[blockIdx.x] = tv;
		wg_p[blockIdx.x] = tp;
	}
}

__global__ void k_iso_totals(const uint64_t* __restrict__ sv, const uint64_t* __restrict__ sp, const uint32_t* __restrict__ flag,
                             int64_t nb, uint64_t* __restrict__ out)
{
	out[0] = sv[nb];
	out[1] = sp[nb];
	out[2] = *flag;
}

// central differences, one-sided at the lattice border
template <int D>
__device__ inline void gradient(const IsoView& v, const int* c, float fc, float* g)
{
	for (int a = 0; a < D; ++a) {
		int lo[3] = {c[0], c[1], c[2]}, hi[3] = {c[0], c[1], c[2]};
		lo[a] -= 1;
		hi[a] += 1;
		const bool has_lo = c[a] > 0, has_hi = c[a] + 1 < v.n[a];
		if (has_lo && has_hi) {
			g[a] = (ld<D>(v, hi) - ld<D>(v, lo)) * 0.5f;
		} else if (has_hi) {
			g[a] = ld<D>(v, hi) - fc;
		} else if (has_lo) {
			g[a] = fc - ld<D>(v, lo);
		} else {
			g[a] = 0.0f;
		}
	}
}

template <int D>
__global__ __launch_bounds__(kIsoThreads) void k_iso_vertices(IsoView v, const uint64_t* __restrict__ wg_off,
                                                              uint32_t* __restrict__ base, float* __restrict__ pos,
                                                              float* __restrict__ nrm, int64_t* __restrict__ key)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kIsoThreads + threadIdx.x;
	int c[3] = {0, 0, 0};
	float fc = 0.0f;
	unsigned m = 0;
	if (i < v.npts) {
		coords<D>(v, i, c);
		fc = ld<D>(v, c);
		bool bad = false;
		m = crossings<D>(v, c, fc, &bad);
	}
	uint32_t total = 0;
	const uint32_t pre = block_scan<kIsoThreads>(__popc(m), &total);
	if (i >= v.npts) { return; }
	uint64_t k = wg_off[blockIdx.x] + pre;
	base[i] = static_cast<uint32_t>(k);
	if (m == 0) { return; }
	float gp[3] = {0, 0, 0};
	gradient<D>(v, c, fc, gp);
	int64_t gidx = c[0] + static_cast<int64_t>(v.n[0]) * (c[1] + static_cast<int64_t>(v.n[1]) * (D == 3 ? c[2] : 0));
	for (int a = 0; a < D; ++a, m >>= 1) {
		if (!(m & 1u)) { continue; }
		int q[3] = {c[0], c[1], c[2]};
		q[a] += 1;
		const float fq = ld<D>(v, q);
		const float dp = fc - v.iso, dq = fq - v.iso;
		const float t  = dp / (dp - dq);
		float gq[3] = {0, 0, 0};
		gradient<D>(v, q, fq, gq);
		float nv[3], len2 = 0.0f;
		for (int d = 0; d < D; ++d) {
			pos[k * D + d] = d == a ? static_cast<float>(c[d]) + t : static_cast<float>(c[d]);
			nv[d] = (1.0f - t) * gp[d] + t * gq[d];
			len2 += nv[d] * nv[d];
		}
		const float len = sqrtf(len2);
		for (int d = 0; d < D; ++d) { nrm[k * D + d] = len > 0.0f ? nv[d] / len : 0.0f; }
		key[k] = D * gidx + a;
		++k;
	}
}

// the vertex on local cell edge e of the cell at c: the base of the edge's lower corner + the crossing edges of that corner
// along the axes before the edge's
template <int D>
__device__ inline int vertex_of(const IsoView& v, const int* c, unsigned cs, int e, const uint32_t* __restrict__ base)
{
	const int a = e >> (D - 1), j = e & ((1 << (D - 1)) - 1);
	int q[3] = {c[0], c[1], c[2]};
	int o = 0;
	for (int b = 0; b < D; ++b) {
		if (b == a) { continue; }
		q[b] += (j >> o) & 1;
		++o;
	}
	const int corner = (q[0] - c[0]) | ((q[1] - c[1]) << 1) | (D == 3 ? (q[2] - c[2]) << 2 : 0);
	const bool in = (cs >> corner) & 1u;
	int rank = 0;
	for (int b = 0; b < a; ++b) {  // (b < a < D: never the slowest axis)
		if (q[b] + 1 >= v.n[b]) { continue; }
		int r[3] = {q[0], q[1], q[2]};
		r[b] += 1;
		rank += (ld<D>(v, r) < v.iso) != in;
	}
	const int64_t li = (q[D - 1] - v.clo) * v.plane + q[0] + (D == 3 ? static_cast<int64_t>(v.n[0]) * q[1] : 0);
	return static_cast<int>(base[li]) + rank;
}

template <int D>
__global__ __launch_bounds__(kIsoThreads) void k_iso_prims(IsoView v, const uint64_t* __restrict__ wg_off,
                                                           const uint32_t* __restrict__ base, int* __restrict__ idx)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kIsoThreads + threadIdx.x;
	int c[3] = {0, 0, 0};
	unsigned cs = 0, np = 0;
	if (i < v.npts) {
		coords<D>(v, i, c);
		if (is_cell<D>(v, c)) {
			cs = cell_case<D>(v, c);
			np = prims_of<D>(cs);
		}
	}
	uint32_t total = 0;
	const uint32_t pre = block_scan<kIsoThreads>(np, &total);
	if (np == 0) { return; }
	const uint64_t k = wg_off[blockIdx.x] + pre;
	for (unsigned t = 0; t < np; ++t) {
		for (int s = 0; s < D; ++s) {
			const int e = D == 2 ? iso::kSqSeg[cs][2 * t + s] : iso::kCubeTri[cs][3 * t + s];
			idx[(k + t) * D + s] = vertex_of<D>(v, c, cs, e, base);
		}
	}
}

template <int D>
void run_view(const IsoView& v0, hipStream_t st, fi_mesh* m)
{
	IsoView v = v0;
	m->ndim = D;
	m->nv = m->np = 0;
	bool empty = v.chi <= v.clo;
	for (int a = 0; a < D; ++a) { empty = empty || v.n[a] < 2; }
	if (empty) { return; }
	v.npts = v.plane * (v.chi - v.clo + 1);
	const int64_t nb = (v.npts + kIsoThreads - 1) / kIsoThreads;
	const dim3    groups(static_cast<unsigned>(nb)), threads(kIsoThreads);
	ExtractScans  s;
	const bool    any = extract_sizes<D>(
		nb, st, m, s,
		[&](uint32_t* wg_v, uint32_t* wg_p, uint32_t* flag) { hipLaunchKernelGGL((k_iso_count<D>), groups, threads, 0, st, v, wg_v, wg_p, flag); },
		[&](const uint64_t* sv, const uint64_t* sp, const uint32_t* flag, uint64_t* tot) {
			hipLaunchKernelGGL(k_iso_totals, dim3(1), dim3(1), 0, st, sv, sp, flag, nb, tot);
		});
	if (!any) { return; }
	DevBuf base;
	base.alloc(sizeof(uint32_t) * v.npts);
	hipLaunchKernelGGL((k_iso_vertices<D>), groups, threads, 0, st, v, s.sv, base.as<uint32_t>(), m->pos.as<float>(), m->nrm.as<float>(),
	                   m->key.as<int64_t>());
	FI_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL((k_iso_prims<D>), groups, threads, 0, st, v, s.sp, base.as<uint32_t>(), m->idx.as<int>());
	FI_HIP_TRY(hipGetLastError());
	FI_HIP_TRY(hipStreamSynchronize(st));
}

// the view of piece [lo, hi) of the slowest axis over a window that starts at global plane `first` of `f`
IsoView piece_view(const float* f, int first, int ndim, const int* sizes, float iso, int lo, int hi)
{
	IsoView v{};
	const int S = sizes[ndim - 1];
	v.plane = 1;
	for (int d = 0; d < 3; ++d) {
		v.n[d] = d < ndim ? sizes[d] : 1;
		if (d < ndim - 1) { v.plane *= sizes[d]; }
	}
	v.clo = lo;
	v.chi = hi < S - 1 ? hi : S - 1;
	v.wlo = lo > 0 ? lo - 1 : 0;
	v.whi = v.chi + 2 < S ? v.chi + 2 : S;
	v.f   = f + (v.wlo - first) * v.plane;
	v.iso = iso;
	return v;
}

void run_any(int ndim, const IsoView& v, hipStream_t st, fi_mesh* m)
{
	m->ndim = ndim;
	if (ndim == 2) {
		run_view<2>(v, st, m);
	} else {
		run_view<3>(v, st, m);
	}
}

struct MeshList {  // meshes made so far, destroyed if a later one fails
	std::vector<fi_mesh*> v;
	~MeshList()
	{
		for (fi_mesh* m : v) { delete m; }
	}
	fi_mesh* add()
	{
		v.push_back(new fi_mesh());
		FI_HIP_TRY(hipGetDevice(&v.back()->device));
		return v.back();
	}
	void hand_out(fi_mesh** out)
	{
		for (size_t r = 0; r < v.size(); ++r) { out[r] = v[r]; }
		v.clear();
	}
};

void check_dims(int ndim, const int* sizes) { check_mesh_dims(ndim, sizes, "iso-contours of a 1-D lattice are not supported"); }

}  // namespace

void iso_extract_whole(const float* field, int ndim, const int* sizes, float iso, int pieces, const int* slab_lo,
                       const int* slab_hi, hipStream_t st, fi_mesh** out)
{
	check_dims(ndim, sizes);
	MeshList ms;
	for (int r = 0; r < pieces; ++r) {
		const IsoView v = piece_view(field, 0, ndim, sizes, iso, slab_lo ? slab_lo[r] : 0, slab_hi ? slab_hi[r] : sizes[ndim - 1]);
		run_any(ndim, v, st, ms.add());
	}
	ms.hand_out(out);
}

namespace {

// The pieces of slab contexts: one per process (RankSet of one, ghost planes over RCCL or the host test transport) or all
// members of a loop-back group (device copies).  fields[r]: member r's owned values (`memory`), or nullptr for its last
// solution.  Each member exchanges the ghost planes its piece reads -- plane lo - 1 (normals), hi (positions) and hi + 1
// (normals) -- in its local layout, rounds them to fp32 and extracts the cells of its slab.  Every rank exchanges the same
// width, decided from facts all ranks share.
void slab_pieces(RankSet& R, const float* const* fields, int memory, float iso, fi_mesh** out)
{
	fi_ctx*     c0 = R[0];
	const Geom& g0 = c0->g;
	const int   L  = g0.ndim - 1;
	check_dims(g0.ndim, g0.gn);
	const int want = 2;
	FI_REQUIRE(c0->halo >= want && g0.gn[L] / c0->nranks >= want, FI_ERR_UNSUPPORTED,
	           "iso extraction over slabs needs %d ghost planes and slabs of at least %d planes (the context stores %d ghost "
	           "planes, the thinnest slab has %d planes)", want, want, c0->halo, g0.gn[L] / c0->nranks);
	AllocStream alloc_on(c0->stream);
	slab_fields(R, fields, memory, want);
	MeshList ms;
	DevBuf   buf;
	for (fi_ctx* c : R) {
		const Geom& g = c->g;
		buf.alloc(sizeof(float) * g.nloc);
		if (c->dtype == FI_F64) {
			hipLaunchKernelGGL((k_to_float<double>), dim3(blocks_for(g.nloc)), dim3(kThreads), 0, c->stream, g.nloc, c->q.as<double>(),
			                   buf.as<float>());
		} else {
			hipLaunchKernelGGL((k_to_float<float>), dim3(blocks_for(g.nloc)), dim3(kThreads), 0, c->stream, g.nloc, c->q.as<float>(),
			                   buf.as<float>());
		}
		FI_HIP_TRY(hipGetLastError());
		const IsoView v = piece_view(buf.as<float>(), g.off[L], g.ndim, g.gn, iso, c->slab_lo, c->slab_hi);
		run_any(g.ndim, v, c->stream, ms.add());  // (synchronises the stream: buf is free for the next member)
	}
	ms.hand_out(out);
}

}  // namespace

void iso_extract_ctx(fi_ctx* c, const float* field, float iso, int memory, fi_mesh** out)
{
	const Geom& g = c->g;
	const int   L = g.ndim - 1;
	check_dims(g.ndim, g.gn);
	FI_REQUIRE(field || c->vectors_ready, FI_ERR_STATE, "no solution yet");
	if (field) { check_memory(memory); }
	if (c->nranks > 1) {
		RankSet R{c};
		slab_pieces(R, &field, memory, iso, out);
		return;
	}
	AllocStream alloc_on(c->stream);
	DevBuf buf;
	const float* f = field_f32(c, field, memory, buf);
	MeshList ms;
	run_any(g.ndim, piece_view(f, 0, g.ndim, g.gn, iso, 0, g.gn[L]), c->stream, ms.add());
	ms.hand_out(out);
}

void iso_extract_group(std::vector<fi_ctx*>& members, const float* whole, float iso, fi_mesh** out)
{
	if (!whole) {  // the members' solutions: the slab path of one process per GPU, ghost planes by device copies
		std::vector<const float*> none(members.size(), nullptr);
		slab_pieces(members, none.data(), FI_HOST, iso, out);
		return;
	}
	// the caller holds the whole lattice: every piece reads its window of it, nothing to exchange
	fi_ctx*     c0 = members[0];
	const Geom& g  = c0->g;
	check_dims(g.ndim, g.gn);
	AllocStream alloc_on(c0->stream);
	int64_t n = 1;
	for (int d = 0; d < g.ndim; ++d) { n *= g.gn[d]; }
	DevBuf buf;
	buf.alloc(sizeof(float) * n);
	FI_HIP_TRY(hipMemcpyAsync(buf.p, whole, sizeof(float) * n, hipMemcpyHostToDevice, c0->stream));
	std::vector<int> lo, hi;
	for (fi_ctx* c : members) {
		lo.push_back(c->slab_lo);
		hi.push_back(c->slab_hi);
	}
	iso_extract_whole(buf.as<float>(), g.ndim, g.gn, iso, static_cast<int>(members.size()), lo.data(), hi.data(), c0->stream, out);
}

}  // namespace fi
