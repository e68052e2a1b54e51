// fi_nearest.hip -- exact nearest data points on the device.
//
// The contract (include/fi_hip.h fi_nearest): s(p, q) is the fp32 sum from 0.0f of (p_d - q_d)^2 in ascending
// d, one rounding per operation (-ffp-contract=off) -- the arithmetic of the reference's border-prior loop; the result of a
// query is sqrtf of the minimum of s over the finite points and the smallest index that reaches it.
//
// Structure and query: fi_bvh.h's tree and stackless walk (the exactness argument is there) over the finite points, leaves of
// kNearestLeaf consecutive points; this file supplies the points as items and their distance.
#include "fi_solver_internal.h"
#include "fi_nearest.h"
#include "fi_bvh.h"

namespace fi {

namespace {

using namespace bvh;

// the items of the build (fi_bvh.h): n points of D floats; usable means finite; stored as float4 (x, y, z, the index as bits)
template <int D>
struct PointItems {
	static constexpr int  kDim = D, kLeaf = kNearestLeaf, kVerts = 1, kSlots = 1, kBoxAxes = 3;
	static constexpr bool kIds = false;
	const float* __restrict__ pos;
	__device__ int load(int64_t i, float* v) const
	{
#pragma unroll
		for (int d = 0; d < D; ++d) { v[d] = pos[i * D + d]; }
		return finite_point<D>(v) ? 0 : 1;
	}
	__device__ void key_point(const float* v, double* m) const
	{
#pragma unroll
		for (int d = 0; d < D; ++d) { m[d] = v[d]; }
	}
	__device__ void store(int64_t i, uint32_t j, const float* v, float4* __restrict__ pts, uint32_t*) const
	{
		float p[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
		for (int d = 0; d < D; ++d) { p[d] = v[d]; }
		pts[i] = make_float4(p[0], p[1], p[2], __uint_as_float(j));
	}
	__device__ static void extend(const float4* __restrict__ pts, int64_t i, float4& lo, float4& hi)
	{
		const float4 p = pts[i];
		lo.x = fminf(lo.x, p.x), lo.y = fminf(lo.y, p.y), lo.z = fminf(lo.z, p.z);
		hi.x = fmaxf(hi.x, p.x), hi.y = fmaxf(hi.y, p.y), hi.z = fmaxf(hi.z, p.z);
	}
	void check(const uint32_t* c, int64_t n) const
	{
		FI_REQUIRE(c[0] <= static_cast<uint64_t>(n), FI_ERR_HIP, "nearest: %u finite points of %lld", c[0], static_cast<long long>(n));
	}
};

// the points the tree leaves out (the non-finite ones), appended in whatever order the integer counter hands out: `room` of
// them at the most
__global__ __launch_bounds__(kThreads) void k_points_rest(int64_t n, int D, const float* __restrict__ pos, int64_t room, uint32_t* count,
                                                            float4* __restrict__ rest)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	float p[3]   = {0.0f, 0.0f, 0.0f};
	bool  finite = true;
	for (int d = 0; d < D; ++d) {
		p[d]   = pos[i * D + d];
		finite = finite && isfinite(p[d]);
	}
	if (finite) { return; }
	const uint32_t at = atomicAdd(count, 1u);
	if (at < room) { rest[at] = make_float4(p[0], p[1], p[2], __uint_as_float(static_cast<uint32_t>(i))); }
}

// where the queries come from
enum { kFromBuffer = 0, kFromLattice = 1, kFromList = 2 };

struct QueryArgs {
	Tree             t;
	int64_t          n;
	const float*     q;        // kFromBuffer: float[n][D]
	Lattice          l;        // kFromLattice / kFromList: the lattice (kFromLattice: and its tiles)
	const uint32_t*  list;     // kFromList: linear lattice indices
	float            lim;      // the largest float whose sqrtf is <= max_distance
	float*           dist;
	long long*       idx;      // or nullptr
	float*           d2;       // kFromList: the squared distance
};

template <int D, int SRC>
__global__ __launch_bounds__(kThreads) void k_nearest_query(QueryArgs a)
{
	float   q[D];
	int64_t out;
	if constexpr (SRC == kFromLattice) {
		if (!lattice_query<D>(a.l, q, &out)) { return; }
	} else {
		out = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
		if (out >= a.n) { return; }
		if constexpr (SRC == kFromList) {
			uint32_t r = a.list[out];
#pragma unroll
			for (int d = 0; d < D; ++d) {
				q[d] = static_cast<float>(r % static_cast<uint32_t>(a.l.sz[d]));
				r /= static_cast<uint32_t>(a.l.sz[d]);
			}
		} else {
#pragma unroll
			for (int d = 0; d < D; ++d) { q[d] = a.q[out * D + d]; }
		}
	}
	const bool finite = finite_point<D>(q);
	float      best   = NAN;
	uint32_t   bidx   = kNone;  // the smallest index that reaches best
	if (finite) {
		search<D, kNearestLeaf>(a.t, q, a.lim, best, [&](int64_t i, float& least) {
			const float4   p = a.t.items[i];
			const float    s = sq_dist<D>(p, q);
			const uint32_t j = __float_as_uint(p.w);
			if (s < least || (s == least && j < bidx)) {
				least = s;
				bidx = j;
			}
		});
	}
	if constexpr (SRC == kFromList) {
		a.d2[out] = best;
		return;
	}
	a.dist[out] = distance_of(finite, best, a.lim, bidx);
	if (a.idx) { a.idx[out] = index_of(bidx); }
}

template <int SRC>
void launch_query(int D, dim3 grid, const QueryArgs& a, hipStream_t st)
{
	switch (D) {
	case 1: hipLaunchKernelGGL((k_nearest_query<1, SRC>), grid, dim3(kThreads), 0, st, a); break;
	case 2: hipLaunchKernelGGL((k_nearest_query<2, SRC>), grid, dim3(kThreads), 0, st, a); break;
	default: hipLaunchKernelGGL((k_nearest_query<3, SRC>), grid, dim3(kThreads), 0, st, a); break;
	}
	FI_HIP_TRY(hipGetLastError());
}

}  // namespace

void nearest_build(NearestIndex& t, int D, int64_t n, const float* const* seg_pos, const int64_t* seg_n, int nseg, hipStream_t st)
{
	t.D  = D;
	t.n  = n;
	t.nf = 0;
	t.H  = 0;
	if (n == 0) { return; }
	FI_REQUIRE(n < (int64_t(1) << 31), FI_ERR_UNSUPPORTED, "%lld points: nearest-point indices are 32-bit", static_cast<long long>(n));
	DevBuf       all;
	const float* pos = seg_pos[0];
	if (nseg > 1) {  // one contiguous set
		all.alloc(sizeof(float) * D * n);
		int64_t at = 0;
		for (int s = 0; s < nseg; ++s) {
			if (seg_n[s] > 0) {
				FI_HIP_TRY(hipMemcpyAsync(all.as<float>() + at * D, seg_pos[s], sizeof(float) * D * seg_n[s], hipMemcpyDeviceToDevice, st));
			}
			at += seg_n[s];
		}
		pos = all.as<float>();
	}
	switch (D) {
	case 1: build(t, PointItems<1>{pos}, n, st); break;
	case 2: build(t, PointItems<2>{pos}, n, st); break;
	default: build(t, PointItems<3>{pos}, n, st); break;
	}
	if (t.nf < n) {  // (a clean set never comes here)
		DevBuf count;
		count.alloc(sizeof(uint32_t));
		t.rest.alloc(sizeof(float4) * (n - t.nf));
		FI_HIP_TRY(hipMemsetAsync(count.p, 0, sizeof(uint32_t), st));
		hipLaunchKernelGGL(k_points_rest, dim3(blocks_for(n)), dim3(kThreads), 0, st, n, D, pos, n - t.nf, count.as<uint32_t>(),
		                   t.rest.as<float4>());
		FI_HIP_TRY(hipGetLastError());
		FI_HIP_TRY(hipStreamSynchronize(st));  // (`all` and the counter die here)
	}
}

const NearestIndex& nearest_of(fi_ctx* c)
{
	if (c->nearest) { return *c->nearest; }
	std::vector<const float*> seg;
	std::vector<int64_t>      cnt;
	int64_t                   n = 0;
	for (const PointBatch* b : c->batches) {
		if (b->n <= 0 || b->prior) { continue; }
		seg.push_back(b->pos.as<float>());
		cnt.push_back(b->n);
		n += b->n;
	}
	NearestIndex* t = new NearestIndex();
	try {
		AllocStream alloc_on(c->stream);
		nearest_build(*t, c->g.ndim, n, seg.data(), cnt.data(), static_cast<int>(seg.size()), c->stream);
	} catch (...) {
		delete t;
		throw;
	}
	c->nearest = t;
	return *t;
}

void nearest_release(fi_ctx* c)
{
	delete c->nearest;
	c->nearest = nullptr;
}

void nearest_query(const NearestIndex& t, int64_t n, const float* queries, float max_distance, float* distances, long long* indices,
                   int memory, hipStream_t st)
{
	if (n == 0) { return; }
	AllocStream alloc_on(st);
	Outputs o(n, t.D, distances, indices, nullptr, memory);
	stage::In<float> q(queries, n * t.D, memory, st);
	QueryArgs a{};
	a.t    = tree_of(t);
	a.n    = n;
	a.q    = q;
	a.lim  = limit_for(max_distance);
	a.dist = o.dist;
	a.idx  = o.idx;
	launch_query<kFromBuffer>(t.D, dim3(blocks_for(n)), a, st);
	o.finish(st);
}

void nearest_lattice(const NearestIndex& t, const int* sizes, float max_distance, float* distances, long long* indices, int memory,
                     hipStream_t st)
{
	QueryArgs   a{};
	int64_t     total = 0;
	const dim3  grid  = lattice_grid(t.D, sizes, a.l, &total);
	AllocStream alloc_on(st);
	Outputs o(total, t.D, distances, indices, nullptr, memory);
	a.t    = tree_of(t);
	a.n    = total;
	a.lim  = limit_for(max_distance);
	a.dist = o.dist;
	a.idx  = o.idx;
	launch_query<kFromLattice>(t.D, grid, a, st);
	o.finish(st);
}

void nearest_lattice_list_d2(const NearestIndex& t, const int* n, int64_t nb, const uint32_t* idx, float* d2, hipStream_t st)
{
	if (nb == 0) { return; }
	QueryArgs a{};
	for (int d = 0; d < 3; ++d) { a.l.sz[d] = d < t.D ? n[d] : 1; }
	a.t    = tree_of(t);
	a.n    = nb;
	a.list = idx;
	a.lim  = INFINITY;
	a.d2   = d2;
	launch_query<kFromList>(t.D, dim3(blocks_for(nb)), a, st);
}

}  // namespace fi
