// fi_mls.hip -- a point cloud made smooth on the device: moving-least-squares projection onto a local plane or quadric.
//
// The contract (include/fi_hip.h fi_mls_project; tests/mls_reference.py is its definition in numpy): a
// query's neighbours are the first k pairs (s, j) of fi_knn's order with sqrtf(s) <= radius; weights (1 - s / h^2)^3 in fp64
// from the fp32 s; the weighted centroid and covariance, fi_jacobi.h's sweeps, the frame of the smallest diagonal entry; the
// quadric's weighted normal equations over local coordinates divided by h, solved by an unpivoted Cholesky in a fixed order;
// the query projected along the frame normal.  Every fp64 figure is one rounding per operation (-ffp-contract=off) over
// + - * / sqrt, every sum from 0.0 in list order.  No atomics: a repeated call returns the same bytes.
//
// How it is found, two kernels (the list of fi_knn_list.h takes up to 96 VGPRs at capacity 32, the fit 27 fp64 sums and a
// frame: one kernel would spill):
//   walk   k_cloud_neighbours' shape: fi_bvh.h's stackless walk over fi_nearest.h's tree, unchanged, fi_knn_list.h's list in
//          the classes 8 / 16 / 32 -- without the entries' sorted slots, which would cost a third register an entry and the
//          walk its occupancy.  It writes each list entry's point index and s into the call's scratch, entry r of thread i
//          at [r * stride + i]: a wave's stores coalesce.  Own points: a thread per SORTED SLOT, as k_knn_normals.
//   fit    a thread per point: reads the entries back in list order (three passes: centroid, covariance, normal equations),
//          fetches the positions from the tree's items through a map from point index to sorted slot (k_mls_slots, 4 bytes a
//          point, made once a call), and keeps everything else in registers.
// The points are taken kMlsChunk at a time, so the lists' scratch is 8 k kMlsChunk bytes at the most: 64 MiB at k = 32.
#include "fi_solver_internal.h"
#include "fi_mls.h"
#include "fi_bvh.h"
#include "fi_knn_list.h"
#include "fi_jacobi.h"
#include "fi_prim.h"

#include <algorithm>

namespace fi {

namespace {

using namespace bvh;
using namespace knn;

constexpr int64_t kMlsChunk = int64_t(1) << 18;  // the points of one walk + fit pair
// a Cholesky pivot of the quadric's normal equations must exceed kMlsPivot W: the geometric middle of the largest ratio on
// degenerate neighbourhoods (1.2e-27, a collinear cloud) and the smallest on a noisy sphere (8.4e-4) -- DESIGN.md 4.25
constexpr double kMlsPivot = 1.0e-15;

struct WalkArgs {
	Tree         t;
	int64_t      base, count;  // this launch's threads stand for the queries / sorted slots [base, base + count)
	int64_t      stride;       // of the scratch: entry r of thread i at [r * stride + i]
	const float* q;            // float[n][D], or unused (SELF)
	int          k;
	float        lim;          // the largest float whose sqrtf is <= radius
	uint32_t*    idx;          // the point index of each list entry; kNone: no such entry (and none behind it)
	float*       s;
};

// where the tree keeps point j: slot_of[j] for the points it holds
__global__ __launch_bounds__(kThreads) void k_mls_slots(Tree t, uint32_t* __restrict__ slot_of)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= t.nf) { return; }
	slot_of[__float_as_uint(t.items[i].w)] = static_cast<uint32_t>(i);
}

template <int D, int CAP, bool SELF>
__global__ __launch_bounds__(kThreads) void k_mls_walk(WalkArgs a)
{
	const int64_t li = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (li >= a.count) { return; }
	const int64_t i = a.base + li;
	float         q[D];
	if constexpr (SELF) {
		const float4 self  = a.t.items[i];
		const float  s3[3] = {self.x, self.y, self.z};
#pragma unroll
		for (int d = 0; d < D; ++d) { q[d] = s3[d]; }
	} else {
#pragma unroll
		for (int d = 0; d < D; ++d) { q[d] = a.q[i * D + d]; }
	}
	List<CAP> b;
	list_reset<CAP>(b, CAP - a.k);
	if (SELF || finite_point<D>(q)) {
		float bound;
		search<D, kNearestLeaf>(a.t, q, a.lim, bound, [&](int64_t at, float& least) {
			const float4 p = a.t.items[at];
			list_offer<CAP>(b, sq_dist<D>(p, q), __float_as_uint(p.w), 0u);
			least = b.s;  // the k-th s: +inf until k pairs are held
		});
	}
	list_each<CAP>(b, [&](int r, float s, uint32_t j, uint32_t) {
		const int o = r - (CAP - a.k);
		if (o < 0) { return; }
		const bool ok = found(s, j, a.lim);
		a.idx[o * a.stride + li] = ok ? j : kNone;
		a.s[o * a.stride + li]   = s;
	});
}

struct FitArgs {
	Tree            t;
	int64_t         base, count, stride;
	const float*    q;       // float[n][D], or unused (SELF)
	int             k;
	double          h;       // the radius
	double          mm;      // max_move
	const uint32_t* idx;
	const uint32_t* slot_of;  // point index -> sorted slot
	const float*    s;
	const float*    guides;  // float[n][D] by output index, or nullptr
	float*          pos;     // float[n][D], or nullptr
	float*          nrm;     // float[n][D], or nullptr
	float*          curv;    // float[n], or nullptr
	unsigned char*  order;   // n bytes, or nullptr
};

template <int D>
__device__ inline double dot0(const double* a, const double* b)
{
	double s = 0.0;
#pragma unroll
	for (int d = 0; d < D; ++d) { s = s + a[d] * b[d]; }
	return s;
}

// the point stays where it is (a NaN for a non-finite query): order 0, a zero normal, a NaN curvature
template <int D>
__device__ inline void mls_stay(const FitArgs& a, int64_t out, const float* q, bool nan)
{
#pragma unroll
	for (int d = 0; d < D; ++d) {
		if (a.pos) { a.pos[out * D + d] = nan ? NAN : q[d]; }
		if (a.nrm) { a.nrm[out * D + d] = 0.0f; }
	}
	if (a.curv) { a.curv[out] = NAN; }
	if (a.order) { a.order[out] = 0; }
}

template <int D, int DEG, bool SELF>
__global__ __launch_bounds__(kThreads) void k_mls_fit(FitArgs a)
{
	constexpr int NB = D == 3 ? 6 : 3;  // the quadric's coefficients
	const int64_t li = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (li >= a.count) { return; }
	const int64_t i   = a.base + li;
	int64_t       out = i;
	float         q[D];
	if constexpr (SELF) {
		const float4 self  = a.t.items[i];
		const float  s3[3] = {self.x, self.y, self.z};
		out                = __float_as_uint(self.w);
#pragma unroll
		for (int d = 0; d < D; ++d) { q[d] = s3[d]; }
	} else {
#pragma unroll
		for (int d = 0; d < D; ++d) { q[d] = a.q[i * D + d]; }
		if (!finite_point<D>(q)) {
			mls_stay<D>(a, out, q, true);
			return;
		}
	}
	const double h = a.h, h2 = h * h;
	// f(w, x): every neighbour in list order with its weight and its position
	auto each = [&](auto&& f) {
		for (int r = 0; r < a.k; ++r) {
			const uint32_t j = a.idx[r * a.stride + li];
			if (j == kNone) { break; }
			double w = 1.0 - static_cast<double>(a.s[r * a.stride + li]) / h2;
			w        = w < 0.0 ? 0.0 : w;
			w        = (w * w) * w;
			const float4 p    = a.t.items[a.slot_of[j]];
			const float  v[3] = {p.x, p.y, p.z};
			double       x[D];
#pragma unroll
			for (int d = 0; d < D; ++d) { x[d] = static_cast<double>(v[d]); }
			f(w, x);
		}
	};

	// the weights' sum and the weighted centroid
	int    m = 0, positive = 0;
	double W = 0.0, c[D];
#pragma unroll
	for (int d = 0; d < D; ++d) { c[d] = 0.0; }
	each([&](double w, const double* x) {
		W = W + w;
#pragma unroll
		for (int d = 0; d < D; ++d) { c[d] = c[d] + w * x[d]; }
		++m;
		positive += w > 0.0 ? 1 : 0;
	});
	if (m < D || positive < D || !(W > 0.0)) {
		mls_stay<D>(a, out, q, false);
		return;
	}
#pragma unroll
	for (int d = 0; d < D; ++d) { c[d] = c[d] / W; }

	// the weighted covariance sums
	double A[D][D], V[D][D];
#pragma unroll
	for (int x = 0; x < D; ++x) {
#pragma unroll
		for (int y = 0; y < D; ++y) {
			A[x][y] = 0.0;
			V[x][y] = x == y ? 1.0 : 0.0;
		}
	}
	each([&](double w, const double* x) {
		double e[D];
#pragma unroll
		for (int d = 0; d < D; ++d) { e[d] = x[d] - c[d]; }
#pragma unroll
		for (int x0 = 0; x0 < D; ++x0) {
			const double we = w * e[x0];
#pragma unroll
			for (int y = x0; y < D; ++y) { A[x0][y] = A[x0][y] + we * e[y]; }
		}
	});
#pragma unroll
	for (int x = 0; x < D; ++x) {
#pragma unroll
		for (int y = 0; y < x; ++y) { A[x][y] = A[y][x]; }
	}
	jacobi::jacobi_sweeps<D>(A, V);

	// the frame: the column of the smallest diagonal entry (the lowest on a tie) with the canonical sign, the others as they are
	int    col  = 0;
	double lmin = A[0][0];
#pragma unroll
	for (int d = 1; d < D; ++d) {
		if (A[d][d] < lmin) {
			lmin = A[d][d];
			col  = d;
		}
	}
	double nr[D], t1[D], t2[D];
#pragma unroll
	for (int d = 0; d < D; ++d) {
		nr[d] = V[d][0];
#pragma unroll
		for (int x = 1; x < D; ++x) { nr[d] = col == x ? V[d][x] : nr[d]; }
		t1[d] = col == 0 ? V[d][1] : V[d][0];
		t2[d] = D == 3 ? (col == 2 ? V[d][1] : V[d][D - 1]) : 0.0;
	}
	double big = nr[0];
#pragma unroll
	for (int d = 1; d < D; ++d) { big = fabs(nr[d]) > fabs(big) ? nr[d] : big; }
	if (big < 0.0) {
#pragma unroll
		for (int d = 0; d < D; ++d) { nr[d] = -nr[d]; }
	}

	// the quadric: the weighted normal equations of z over the basis, an unpivoted Cholesky
	double x[NB];
#pragma unroll
	for (int b = 0; b < NB; ++b) { x[b] = 0.0; }
	int order = 1;
	if constexpr (DEG == 2) {
		if (m >= NB) {
			double M[NB][NB], rhs[NB];  // M: the upper triangle holds the sums, the lower one the factor
#pragma unroll
			for (int r = 0; r < NB; ++r) {
				rhs[r] = 0.0;
#pragma unroll
				for (int s = 0; s < NB; ++s) { M[r][s] = 0.0; }
			}
			each([&](double w, const double* p) {
				double e[D];
#pragma unroll
				for (int d = 0; d < D; ++d) { e[d] = p[d] - c[d]; }
				const double u = dot0<D>(e, t1) / h;
				const double z = dot0<D>(e, nr) / h;
				double       B[NB];
				B[0] = 1.0;
				B[1] = u;
				if constexpr (D == 3) {
					const double v = dot0<D>(e, t2) / h;
					B[2] = v;
					B[3] = u * u;
					B[4] = u * v;
					B[5] = v * v;
				} else {
					B[2] = u * u;
				}
#pragma unroll
				for (int r = 0; r < NB; ++r) {
					const double wb = w * B[r];
#pragma unroll
					for (int s = r; s < NB; ++s) { M[r][s] = M[r][s] + wb * B[s]; }
					rhs[r] = rhs[r] + wb * z;
				}
			});
			const double floor_ = kMlsPivot * W;
			bool         ok     = true;
#pragma unroll
			for (int j = 0; j < NB; ++j) {
				double d = M[j][j];
#pragma unroll
				for (int k = 0; k < j; ++k) { d = d - M[j][k] * M[j][k]; }
				ok = ok && d > floor_;
				const double l = sqrt(d);
#pragma unroll
				for (int r = j + 1; r < NB; ++r) {
					double t = M[j][r];
#pragma unroll
					for (int k = 0; k < j; ++k) { t = t - M[r][k] * M[j][k]; }
					M[r][j] = t / l;
				}
				M[j][j] = l;
			}
			double y[NB];
#pragma unroll
			for (int r = 0; r < NB; ++r) {
				double t = rhs[r];
#pragma unroll
				for (int k = 0; k < r; ++k) { t = t - M[r][k] * y[k]; }
				y[r] = t / M[r][r];
			}
			double sol[NB];
#pragma unroll
			for (int r = NB - 1; r >= 0; --r) {
				double t = y[r];
#pragma unroll
				for (int k = r + 1; k < NB; ++k) { t = t - M[k][r] * sol[k]; }
				sol[r] = t / M[r][r];
			}
			if (ok) {
				order = 2;
#pragma unroll
				for (int b = 0; b < NB; ++b) { x[b] = sol[b]; }
			}
		}
	}

	// the query in the frame, its foot on the graph of p, the graph's normal and curvature there
	double eq[D];
#pragma unroll
	for (int d = 0; d < D; ++d) { eq[d] = static_cast<double>(q[d]) - c[d]; }
	const double u0 = dot0<D>(eq, t1) / h;
	double       xp[D], g[D], curv;
	if constexpr (D == 3) {
		const double v0 = dot0<D>(eq, t2) / h;
		double       p  = x[0] + x[1] * u0;
		p               = p + x[2] * v0;
		p               = p + x[3] * (u0 * u0);
		p               = p + x[4] * (u0 * v0);
		p               = p + x[5] * (v0 * v0);
		double pu       = x[1] + (2.0 * x[3]) * u0;
		pu              = pu + x[4] * v0;
		double pv       = x[2] + x[4] * u0;
		pv              = pv + (2.0 * x[5]) * v0;
		const double puu = 2.0 * x[3], puv = x[4], pvv = 2.0 * x[5];
#pragma unroll
		for (int d = 0; d < D; ++d) {
			xp[d] = c[d] + h * ((u0 * t1[d] + v0 * t2[d]) + p * nr[d]);
			g[d]  = (nr[d] - pu * t1[d]) - pv * t2[d];
		}
		const double a1 = 1.0 + pu * pu, b1 = 1.0 + pv * pv;
		const double gg  = a1 + pv * pv;
		const double num = (b1 * puu - ((2.0 * pu) * pv) * puv) + a1 * pvv;
		curv             = num / ((2.0 * h) * (gg * sqrt(gg)));
	} else {
		double p        = x[0] + x[1] * u0;
		p               = p + x[2] * (u0 * u0);
		const double pu = x[1] + (2.0 * x[2]) * u0;
		const double puu = 2.0 * x[2];
#pragma unroll
		for (int d = 0; d < D; ++d) {
			xp[d] = c[d] + h * (u0 * t1[d] + p * nr[d]);
			g[d]  = nr[d] - pu * t1[d];
		}
		const double gg = 1.0 + pu * pu;
		curv            = puu / (h * (gg * sqrt(gg)));
	}
	if (order != 2) { curv = 0.0; }
	double l2 = g[0] * g[0];
#pragma unroll
	for (int d = 1; d < D; ++d) { l2 = l2 + g[d] * g[d]; }
	const double len = sqrt(l2);
#pragma unroll
	for (int d = 0; d < D; ++d) { g[d] = g[d] / len; }
	if (a.guides) {
		double gd[D];
#pragma unroll
		for (int d = 0; d < D; ++d) { gd[d] = static_cast<double>(a.guides[out * D + d]); }
		const double w = dot0<D>(g, gd);
		if (isfinite(w) && w < 0.0) {
#pragma unroll
			for (int d = 0; d < D; ++d) { g[d] = -g[d]; }
			curv = -curv;
		}
	}
	// max_move: fi_mesh_smooth's rule
	double dl[D];
#pragma unroll
	for (int d = 0; d < D; ++d) { dl[d] = xp[d] - static_cast<double>(q[d]); }
	double s2 = dl[0] * dl[0] + dl[1] * dl[1];
	if constexpr (D == 3) { s2 = s2 + dl[2] * dl[2]; }
	if (s2 > a.mm * a.mm) {
		const double r = a.mm / sqrt(s2);
#pragma unroll
		for (int d = 0; d < D; ++d) { xp[d] = static_cast<double>(q[d]) + dl[d] * r; }
	}
	bool good = isfinite(curv);
#pragma unroll
	for (int d = 0; d < D; ++d) { good = good && isfinite(xp[d]) && isfinite(g[d]); }
	if (!good) {
		mls_stay<D>(a, out, q, false);
		return;
	}
#pragma unroll
	for (int d = 0; d < D; ++d) {
		if (a.pos) { a.pos[out * D + d] = static_cast<float>(xp[d]); }
		if (a.nrm) { a.nrm[out * D + d] = static_cast<float>(g[d]); }
	}
	if (a.curv) { a.curv[out] = static_cast<float>(curv); }
	if (a.order) { a.order[out] = static_cast<unsigned char>(order); }
}

// what a point outside the tree (a non-finite one) gets: its own bits back
__global__ __launch_bounds__(kThreads) void k_mls_rest(int64_t count, int D, const float4* __restrict__ rest, float* __restrict__ pos,
                                                        float* __restrict__ nrm, float* __restrict__ curv, unsigned char* __restrict__ order)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= count) { return; }
	const float4  p    = rest[i];
	const float   v[3] = {p.x, p.y, p.z};
	const int64_t out  = __float_as_uint(p.w);
	for (int d = 0; d < D; ++d) {
		if (pos) { pos[out * D + d] = v[d]; }
		if (nrm) { nrm[out * D + d] = 0.0f; }
	}
	if (curv) { curv[out] = NAN; }
	if (order) { order[out] = 0; }
}

template <int D, bool SELF>
void launch_walk(int cap, dim3 grid, const WalkArgs& a, hipStream_t st)
{
	switch (cap) {
	case 8: hipLaunchKernelGGL((k_mls_walk<D, 8, SELF>), grid, dim3(kThreads), 0, st, a); break;
	case 16: hipLaunchKernelGGL((k_mls_walk<D, 16, SELF>), grid, dim3(kThreads), 0, st, a); break;
	default: hipLaunchKernelGGL((k_mls_walk<D, 32, SELF>), grid, dim3(kThreads), 0, st, a); break;
	}
}

template <int D, bool SELF>
void launch_pair(int cap, int degree, dim3 grid, const WalkArgs& w, const FitArgs& f, hipStream_t st)
{
	launch_walk<D, SELF>(cap, grid, w, st);
	if (degree == 2) {
		hipLaunchKernelGGL((k_mls_fit<D, 2, SELF>), grid, dim3(kThreads), 0, st, f);
	} else {
		hipLaunchKernelGGL((k_mls_fit<D, 1, SELF>), grid, dim3(kThreads), 0, st, f);
	}
}

}  // namespace

void mls_project(const NearestIndex& t, int64_t n, const float* queries, int k, float radius, int degree, float max_move,
                 const float* guide_normals, float* positions, float* normals, float* curvature, unsigned char* order, int memory,
                 hipStream_t st)
{
	const bool self = queries == nullptr;
	if (self) { n = t.n; }
	if (n == 0) { return; }
	AllocStream               alloc_on(st);
	stage::Out<float>         po(positions, n * t.D, memory);
	stage::Out<float>         nr(normals, n * t.D, memory);
	stage::Out<float>         cu(curvature, n, memory);
	stage::Out<unsigned char> od(order, n, memory);
	stage::In<float>          q(queries, n * t.D, memory, st);
	stage::In<float>          g(guide_normals, n * t.D, memory, st);
	const int64_t             total  = self ? t.nf : n;  // the threads: the tree's sorted slots, or the queries
	const int64_t             stride = std::min(total, kMlsChunk);
	uint32_t *                idx = nullptr, *slot_of = nullptr;
	float*                    s   = nullptr;
	DevBuf                    block;
	prim::arena_alloc(block, [&](prim::Arena& a) {
		idx     = a.take<uint32_t>(stride * k);
		s       = a.take<float>(stride * k);
		slot_of = a.take<uint32_t>(t.n);
	});
	WalkArgs w{};
	w.t      = tree_of(t);
	w.stride = stride;
	w.q      = q;
	w.k      = k;
	w.lim    = limit_for(radius);
	w.idx    = idx;
	w.s      = s;
	FitArgs f{};
	f.t      = w.t;
	f.stride = stride;
	f.q      = q;
	f.k      = k;
	f.h      = static_cast<double>(radius);
	f.mm     = static_cast<double>(max_move);
	f.idx     = idx;
	f.slot_of = slot_of;
	f.s       = s;
	f.guides = g;
	f.pos    = po;
	f.nrm    = nr;
	f.curv   = cu;
	f.order  = od;
	if (self && t.nf < t.n) {
		hipLaunchKernelGGL(k_mls_rest, dim3(blocks_for(t.n - t.nf)), dim3(kThreads), 0, st, t.n - t.nf, t.D, t.rest.as<float4>(), f.pos, f.nrm,
		                   f.curv, f.order);
	}
	if (t.nf > 0) { hipLaunchKernelGGL(k_mls_slots, dim3(blocks_for(t.nf)), dim3(kThreads), 0, st, w.t, slot_of); }
	const int cap = capacity_for(k);
	for (int64_t base = 0; base < total; base += kMlsChunk) {
		w.base = f.base = base;
		w.count = f.count = std::min(kMlsChunk, total - base);
		const dim3 grid(blocks_for(w.count));
		if (t.D == 2) {
			if (self) {
				launch_pair<2, true>(cap, degree, grid, w, f, st);
			} else {
				launch_pair<2, false>(cap, degree, grid, w, f, st);
			}
		} else {
			if (self) {
				launch_pair<3, true>(cap, degree, grid, w, f, st);
			} else {
				launch_pair<3, false>(cap, degree, grid, w, f, st);
			}
		}
		FI_HIP_TRY(hipGetLastError());
	}
	po.back(st);
	nr.back(st);
	cu.back(st);
	od.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

}  // namespace fi
