// fi_knn.hip -- exact k nearest data points, and point-cloud normals from them, on the device.
//
// The contract (include/fi_hip.h fi_knn / fi_estimate_normals): s(p, q) is fi_nearest's; a query's result is
// the first k of the pairs (s, j) over the finite points in lexicographic order, those beyond max_distance dropped.  A normal
// is the direction of least spread of a point's own k nearest points (itself included): fp64, one rounding per operation
// (-ffp-contract=off), a cyclic Jacobi iteration of a fixed number of sweeps -- the arithmetic of tests/normals_reference.py,
// bit for bit.
//
// Search: fi_bvh.h's stackless walk over fi_nearest.h's tree, unchanged.  The visitor keeps the k best pairs sorted in
// registers and reports the k-th s as the walk's pruning bound; the walk prunes on lb > bound (strict), so a leaf that holds
// an equal s with a smaller index is still visited.  The list has a capacity fixed at compile time (8, 16 or 32) and every
// access names its entry at compile time: an index known at run time would put it in scratch.  A k below the capacity
// blocks the front of the list with entries that sort before every real pair, so the k-th best is always the LAST entry.
#include "fi_solver_internal.h"
#include "fi_knn.h"
#include "fi_bvh.h"
#include "fi_knn_list.h"
#include "fi_jacobi.h"

namespace fi {

namespace {

using namespace bvh;
using namespace knn;  // the list of the k best pairs, capacity_for (fi_knn_list.h)

struct KnnArgs {
	Tree         t;
	int64_t      n;
	const float* q;     // float[n][D]
	int          k;
	float        lim;   // the largest float whose sqrtf is <= max_distance
	float*       dist;  // float[n][k]
	long long*   idx;   // long long[n][k], or nullptr
};

// (the walk is latency-bound: the classes up to 16 stay within 64 VGPRs, 8 waves per SIMD, like fi_nearest's queries --
// tests/test_knn_resources.py)
template <int D, int CAP>
__global__ __launch_bounds__(kThreads) void k_knn_query(KnnArgs a)
{
	const int64_t out = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (out >= a.n) { return; }
	float q[D];
#pragma unroll
	for (int d = 0; d < D; ++d) { q[d] = a.q[out * D + d]; }
	const bool finite = finite_point<D>(q);
	List<CAP>  b;
	list_reset<CAP>(b, CAP - a.k);
	if (finite) {
		float bound;
		search<D, kNearestLeaf>(a.t, q, a.lim, bound, [&](int64_t i, float& least) {
			const float4 p = a.t.items[i];
			list_offer<CAP>(b, sq_dist<D>(p, q), __float_as_uint(p.w), 0u);
			least = b.s;  // the k-th s: +inf until k pairs are held
		});
	}
	list_each<CAP>(b, [&](int r, float s, uint32_t j, uint32_t) {
		const int o = r - (CAP - a.k);
		if (o < 0) { return; }
		const bool ok = finite && found(s, j, a.lim);
		// (a finite point whose s overflows is still a neighbour: +inf with its index, as in fi_nearest)
		a.dist[out * a.k + o] = !finite ? NAN : (ok ? sqrtf(s) : INFINITY);
		if (a.idx) { a.idx[out * a.k + o] = ok ? static_cast<long long>(j) : -1LL; }
	});
}

// ---- normals ----------------------------------------------------------------------------------------------------------

enum { kOrientNone = 0, kOrientViewpoints = 1, kOrientDirections = 2 };

struct NormalArgs {
	Tree         t;
	int          k;
	float        lim;
	int          orient;
	const float* guides;      // float[num_guides][D], or nullptr
	int64_t      num_guides;
	float*       normals;     // float[n][D]
	float*       variation;   // float[n], or nullptr
};

// Thread i takes the point of sorted slot i (a wave's points are Morton neighbours and walk the same nodes), searches its
// neighbours, and fits their plane; the result goes to the point's own index.
template <int D, int CAP>
__global__ __launch_bounds__(kThreads) void k_knn_normals(NormalArgs a)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= a.t.nf) { return; }
	const float4  self = a.t.items[i];
	const float   s3[3] = {self.x, self.y, self.z};
	const int64_t me    = __float_as_uint(self.w);
	float         q[D];
#pragma unroll
	for (int d = 0; d < D; ++d) { q[d] = s3[d]; }
	List<CAP> b;
	list_reset<CAP>(b, CAP - a.k);
	float bound;
	search<D, kNearestLeaf>(a.t, q, a.lim, bound, [&](int64_t at, float& least) {
		const float4 p = a.t.items[at];
		list_offer<CAP>(b, sq_dist<D>(p, q), __float_as_uint(p.w), static_cast<uint32_t>(at));
		least = b.s;
	});

	// the centroid: the neighbours' sum from 0.0 in result order, divided by their number
	int    m = 0;
	double c[D];
#pragma unroll
	for (int d = 0; d < D; ++d) { c[d] = 0.0; }
	list_each<CAP>(b, [&](int, float s, uint32_t j, uint32_t at) {
		if (!found(s, j, a.lim)) { return; }
		const float4 p = a.t.items[at];
		const float  v[3] = {p.x, p.y, p.z};
#pragma unroll
		for (int d = 0; d < D; ++d) { c[d] = c[d] + static_cast<double>(v[d]); }
		++m;
	});
	if (m < D) {  // no plane: a zero normal (the blank fill has written it for the points outside the tree)
#pragma unroll
		for (int d = 0; d < D; ++d) { a.normals[me * D + d] = 0.0f; }
		if (a.variation) { a.variation[me] = NAN; }
		return;
	}
#pragma unroll
	for (int d = 0; d < D; ++d) { c[d] = c[d] / static_cast<double>(m); }

	// the covariance sums, from 0.0 in result order
	double A[D][D], V[D][D];
#pragma unroll
	for (int x = 0; x < D; ++x) {
#pragma unroll
		for (int y = 0; y < D; ++y) {
			A[x][y] = 0.0;
			V[x][y] = x == y ? 1.0 : 0.0;
		}
	}
	list_each<CAP>(b, [&](int, float s, uint32_t j, uint32_t at) {
		if (!found(s, j, a.lim)) { return; }
		const float4 p = a.t.items[at];
		const float  v[3] = {p.x, p.y, p.z};
		double       e[D];
#pragma unroll
		for (int d = 0; d < D; ++d) { e[d] = static_cast<double>(v[d]) - c[d]; }
#pragma unroll
		for (int x = 0; x < D; ++x) {
#pragma unroll
			for (int y = x; y < D; ++y) { A[x][y] = A[x][y] + e[x] * e[y]; }
		}
	});
#pragma unroll
	for (int x = 0; x < D; ++x) {
#pragma unroll
		for (int y = 0; y < x; ++y) { A[x][y] = A[y][x]; }
	}

	jacobi::jacobi_sweeps<D>(A, V);

	// the column of the smallest diagonal entry (the lowest on a tie) ...
	int    col  = 0;
	double lmin = A[0][0];
#pragma unroll
	for (int d = 1; d < D; ++d) {
		if (A[d][d] < lmin) {
			lmin = A[d][d];
			col  = d;
		}
	}
	double nrm[D];
#pragma unroll
	for (int d = 0; d < D; ++d) {
		nrm[d] = V[d][0];
#pragma unroll
		for (int x = 1; x < D; ++x) { nrm[d] = col == x ? V[d][x] : nrm[d]; }
	}
	// ... its component of largest magnitude (the first such axis) made positive
	double big = nrm[0];
#pragma unroll
	for (int d = 1; d < D; ++d) { big = fabs(nrm[d]) > fabs(big) ? nrm[d] : big; }
	bool flip = big < 0.0;
	if (a.orient != kOrientNone) {
		double w = 0.0;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			double g;
			if (a.orient == kOrientViewpoints) {
				g = static_cast<double>(a.guides[(a.num_guides == 1 ? 0 : me) * D + d]) - static_cast<double>(q[d]);
			} else {
				g = static_cast<double>(a.guides[me * D + d]);
			}
			w = w + (flip ? -nrm[d] : nrm[d]) * g;
		}
		if (isfinite(w) && w < 0.0) { flip = !flip; }
	}
#pragma unroll
	for (int d = 0; d < D; ++d) { a.normals[me * D + d] = static_cast<float>(flip ? -nrm[d] : nrm[d]); }
	if (a.variation) {
		double tot = 0.0;
#pragma unroll
		for (int d = 0; d < D; ++d) { tot = tot + A[d][d]; }
		a.variation[me] = static_cast<float>(tot == 0.0 ? 0.0 : lmin / tot);
	}
}

// what a point outside the tree (a non-finite one) gets
__global__ __launch_bounds__(kThreads) void k_knn_blank(int64_t n, int D, float* __restrict__ normals, float* __restrict__ variation)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	for (int d = 0; d < D; ++d) { normals[i * D + d] = 0.0f; }
	if (variation) { variation[i] = NAN; }
}

template <int D>
void launch_query(int cap, dim3 grid, const KnnArgs& a, hipStream_t st)
{
	switch (cap) {
	case 8: hipLaunchKernelGGL((k_knn_query<D, 8>), grid, dim3(kThreads), 0, st, a); break;
	case 16: hipLaunchKernelGGL((k_knn_query<D, 16>), grid, dim3(kThreads), 0, st, a); break;
	default: hipLaunchKernelGGL((k_knn_query<D, 32>), grid, dim3(kThreads), 0, st, a); break;
	}
}

template <int D>
void launch_normals(int cap, dim3 grid, const NormalArgs& a, hipStream_t st)
{
	switch (cap) {
	case 8: hipLaunchKernelGGL((k_knn_normals<D, 8>), grid, dim3(kThreads), 0, st, a); break;
	case 16: hipLaunchKernelGGL((k_knn_normals<D, 16>), grid, dim3(kThreads), 0, st, a); break;
	default: hipLaunchKernelGGL((k_knn_normals<D, 32>), grid, dim3(kThreads), 0, st, a); break;
	}
}

}  // namespace

void knn_query(const NearestIndex& t, int64_t n, const float* queries, int k, float max_distance, float* distances, long long* indices,
               int memory, hipStream_t st)
{
	if (n == 0) { return; }
	AllocStream           alloc_on(st);
	stage::Out<float>     d(distances, n * k, memory);
	stage::Out<long long> ix(indices, n * k, memory);
	stage::In<float>      q(queries, n * t.D, memory, st);
	KnnArgs               a{};
	a.t    = tree_of(t);
	a.n    = n;
	a.q    = q;
	a.k    = k;
	a.lim  = limit_for(max_distance);
	a.dist = d;
	a.idx  = ix;
	const dim3 grid(blocks_for(n));
	switch (t.D) {
	case 1: launch_query<1>(capacity_for(k), grid, a, st); break;
	case 2: launch_query<2>(capacity_for(k), grid, a, st); break;
	default: launch_query<3>(capacity_for(k), grid, a, st); break;
	}
	FI_HIP_TRY(hipGetLastError());
	d.back(st);
	ix.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

void estimate_normals(const NearestIndex& t, int k, float max_distance, int orient, const float* guides, int64_t num_guides,
                      float* normals, float* variation, int memory, hipStream_t st)
{
	if (t.n == 0) { return; }
	AllocStream       alloc_on(st);
	stage::Out<float> nr(normals, t.n * t.D, memory);
	stage::Out<float> va(variation, t.n, memory);
	stage::In<float>  g(orient == kOrientNone ? nullptr : guides, num_guides * t.D, memory, st);
	NormalArgs        a{};
	a.t          = tree_of(t);
	a.k          = k;
	a.lim        = limit_for(max_distance);
	a.orient     = orient;
	a.guides     = g;
	a.num_guides = num_guides;
	a.normals    = nr;
	a.variation  = va;
	if (t.nf < t.n) {
		hipLaunchKernelGGL(k_knn_blank, dim3(blocks_for(t.n)), dim3(kThreads), 0, st, t.n, t.D, a.normals, a.variation);
	}
	if (t.nf > 0) {
		const dim3 grid(blocks_for(t.nf));
		if (t.D == 2) {
			launch_normals<2>(capacity_for(k), grid, a, st);
		} else {
			launch_normals<3>(capacity_for(k), grid, a, st);
		}
	}
	FI_HIP_TRY(hipGetLastError());
	nr.back(st);
	va.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

}  // namespace fi
