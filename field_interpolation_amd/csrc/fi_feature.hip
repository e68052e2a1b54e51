// fi_feature.hip -- what a point's neighbourhood looks like, as 33 numbers that do not change when the cloud is turned or
// shifted (Rusu's fast point feature histograms), and the nearest descriptor of another cloud for every descriptor of one:
// the matched pairs fi_align.hip takes.
//
// The contract (include/fi_hip.h fi_points_describe / fi_feature_match; tests/feature_reference.py is its
// definition in numpy).  Descriptors: fp64 from the fp32 positions and normals, one rounding per operation
// (-ffp-contract=off) over + - * / sqrt, fabs and compares -- no trigonometry: the third feature is a pseudo-angle -- integer
// counts, every sum in a fixed order.  Matching: the squared distance of two rows summed in fp32 over ascending columns by
// ONE lane, the smallest index among equal distances.  No float atomics: a repeated call returns the same bytes.
//
// How a descriptor is found:
//   table      the set's own points, in the tree's order, as the queries of fi::knn_query (as fi_orient.hip does): a wave's
//              queries are Morton neighbours and walk the same nodes.
//   k_feat_live   per point: live or not, and the unit normal in fp64.
//   k_feat_spfh   one thread per point over its row of the table: the three features of every counted pair, binned.  A
//              register array of 33 counters indexed by a run-time bin would go to scratch, so the 11 bins of a feature are
//              5 bits each in one 64-bit word: word[f] += 1 << 5 b.  Three words and the pair count: 32 bytes a point.  A
//              list has at most 32 places, and the point's own entry usually takes one, so a counter is at most 31 -- but
//              the search orders by the fp32 squared distance, which is 0 for distinct points closer than about 1e-23, so
//              32 lower-numbered points there displace the point itself and all 32 pairs count.  A counter then reaches 32
//              only when every pair of the point falls into its bin: the add carries into the next field (or, from bin
//              10, into bit 55) and the word is exactly 1 << 5 (b + 1).  count_of() reads that form back: it is told apart
//              from a true single count by the fields' sum, which is 32 for a word that did not carry.
//   k_feat_fpfh   one thread per point: gathers its neighbours' words, unpacks them with compile-time shifts into 33 fp64
//              accumulators, weights by 1 / squared distance, normalises each block of 11 to 100.
// How a match is found:
//   k_feat_match  a LANE OWNS A ROW OF a in registers; a workgroup of 256 lanes stages a tile of 256 rows of b in LDS (NaN rows
//              for masked, non-finite and padding rows: they compare false) and every lane walks the tile by broadcast
//              reads.  The grid also splits b: a workgroup's best merges into a 64-bit word (bits of s) << 32 | j a row by an
//              integer atomicMin -- s >= 0, so the bits order as the values, and the answer is the same in any order.
//              MFMA is not used: the contract fixes the order of the sum, a matrix instruction does not.
//   k_feat_match_out  the word as index and sqrtf(s); -1 and +inf for a masked or non-finite row of a or no admissible j.
#include "fi_solver_internal.h"
#include "fi_feature.h"
#include "fi_bvh.h"
#include "fi_knn.h"
#include "fi_prim.h"

#include <algorithm>

namespace fi {
namespace {

using namespace bvh;
using prim::Arena;
using prim::arena_alloc;

constexpr int kBins  = 11;  // per feature
constexpr int kWidth = 33;  // FI_FEATURE_WIDTH
constexpr int kTile  = 256; // the rows of b a workgroup stages at a time
static_assert(kWidth == FI_FEATURE_WIDTH && kWidth == 3 * kBins, "three features of eleven bins");
static_assert(kTile == kThreads, "one lane per staged row");
static_assert(kMaxNeighbours <= 32, "a 5-bit counter carries only at 32, when every pair of a full list falls into one bin: count_of()");

struct FeatArgs {
	int64_t              n, nf;
	int                  k;
	const uint32_t*      who;     // [nf] the point of a row of the table
	const long long*     idx;     // [nf][k]
	const float*         pos;     // float[n][3], NaN for a point outside the tree
	const float*         normals; // float[n][3]
	unsigned char*       live;    // [n]
	double*              unit;    // double[n][3]
	unsigned long long*  packed;  // [n][4]: the three words and the pair count
	float*               features;
	unsigned char*       valid;   // or null
};

// the set's positions in point order (the points outside the tree stay NaN, which the fill wrote) and, as the queries of
// the table, in the tree's own order; who[r] is the point of sorted slot r
__global__ __launch_bounds__(kThreads) void k_feat_positions(Tree t, float* __restrict__ pos, float* __restrict__ queries,
                                                              uint32_t* __restrict__ who)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= t.nf) { return; }
	const float4  p    = t.items[i];
	const float   v[3] = {p.x, p.y, p.z};
	const int64_t me   = __float_as_uint(p.w);
	who[i]             = static_cast<uint32_t>(me);
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		pos[me * 3 + d]    = v[d];
		queries[i * 3 + d] = v[d];
	}
}

__global__ __launch_bounds__(kThreads) void k_feat_live(FeatArgs a)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= a.n) { return; }
	bool   ok = true;
	double v[3];
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		const float f = a.normals[i * 3 + d];
		ok            = ok && isfinite(a.pos[i * 3 + d]) && isfinite(f);
		v[d]          = static_cast<double>(f);
	}
	const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
	ok               = ok && isfinite(len) && len > 0.0;
	a.live[i]        = ok ? 1 : 0;
#pragma unroll
	for (int d = 0; d < 3; ++d) { a.unit[i * 3 + d] = ok ? v[d] / len : 0.0; }
}

__device__ inline double dot3(const double (&u)[3], const double (&w)[3]) { return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]; }

__device__ inline void cross3(const double (&u)[3], const double (&w)[3], double (&g)[3])
{
	g[0] = u[1] * w[2] - u[2] * w[1];
	g[1] = u[2] * w[0] - u[0] * w[2];
	g[2] = u[0] * w[1] - u[1] * w[0];
}

__device__ inline void load3(const float* __restrict__ p, int64_t i, double (&x)[3])
{
#pragma unroll
	for (int d = 0; d < 3; ++d) { x[d] = static_cast<double>(p[i * 3 + d]); }
}

__device__ inline void load3(const double* __restrict__ p, int64_t i, double (&x)[3])
{
#pragma unroll
	for (int d = 0; d < 3; ++d) { x[d] = p[i * 3 + d]; }
}

// entry e of point i's row: the neighbour j and w = |p_j - p_i|^2, false when the entry is skipped
__device__ inline bool neighbour(const FeatArgs& a, int64_t i, long long j, const double (&pi)[3], double (&dp)[3], double& w)
{
	if (j < 0 || j == i || !a.live[j]) { return false; }
	double pj[3];
	load3(a.pos, j, pj);
#pragma unroll
	for (int d = 0; d < 3; ++d) { dp[d] = pj[d] - pi[d]; }
	w = (dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2];
	return w != 0.0;
}

// a word of 11 five-bit counters that count m pairs between them: did one of them reach 32 and carry?
__device__ inline bool carried(unsigned long long word, unsigned long long m)
{
	if (m != 32) { return false; }
	unsigned sum = 0;
#pragma unroll
	for (int b = 0; b < kBins; ++b) { sum += static_cast<unsigned>((word >> (5 * b)) & 31ull); }
	return sum != 32;
}

// counter b of the word; of a word that carried, 32 for the bin below the carry bit and 0 elsewhere
__device__ inline double count_of(unsigned long long word, int b, bool over)
{
	return over ? 32.0 * static_cast<double>((word >> (5 * (b + 1))) & 1ull) : static_cast<double>((word >> (5 * b)) & 31ull);
}

__device__ inline int bin_of(double t) { return t < 0.0 ? 0 : t >= 11.0 ? 10 : static_cast<int>(t); }

__global__ __launch_bounds__(kThreads) void k_feat_spfh(FeatArgs a)
{
	const int64_t r = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (r >= a.nf) { return; }
	const int64_t i = a.who[r];
	if (!a.live[i]) { return; }  // (the words stay zero)
	double pi[3], ni[3];
	load3(a.pos, i, pi);
	load3(a.unit, i, ni);
	unsigned long long word[3] = {0ull, 0ull, 0ull}, m = 0;
	for (int e = 0; e < a.k; ++e) {
		const long long j = a.idx[r * a.k + e];
		double          dp[3], w;
		if (!neighbour(a, i, j, pi, dp, w)) { continue; }
		double       nj[3], dir[3];
		const double L = sqrt(w);
		load3(a.unit, j, nj);
#pragma unroll
		for (int d = 0; d < 3; ++d) { dir[d] = dp[d] / L; }
		const double ai = dot3(ni, dir), aj = dot3(nj, dir);
		const bool   swap = fabs(ai) < fabs(aj);
		double       ns[3], nt[3];
#pragma unroll
		for (int d = 0; d < 3; ++d) {
			ns[d]  = swap ? nj[d] : ni[d];
			nt[d]  = swap ? ni[d] : nj[d];
			dir[d] = swap ? -dir[d] : dir[d];
		}
		const double f2 = swap ? -aj : ai;
		double       v[3], u[3];
		cross3(dir, ns, v);
		const double l = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
		if (!(isfinite(l) && l > 0.0)) { continue; }
#pragma unroll
		for (int d = 0; d < 3; ++d) { v[d] = v[d] / l; }
		cross3(ns, v, u);
		const double f1 = dot3(v, nt), x = dot3(ns, nt), y = dot3(u, nt);
		const double s  = fabs(x) + fabs(y);
		const double q  = s > 0.0 ? y / s : 0.0;
		const double f3 = x >= 0.0 ? q : (y >= 0.0 ? 2.0 - q : -2.0 - q);
		if (!(isfinite(f1) && isfinite(f2) && isfinite(f3))) { continue; }
		word[0] += 1ull << (5 * bin_of((f1 + 1.0) * 5.5));
		word[1] += 1ull << (5 * bin_of((f2 + 1.0) * 5.5));
		word[2] += 1ull << (5 * bin_of((f3 + 2.0) * 2.75));
		m += 1;
	}
#pragma unroll
	for (int f = 0; f < 3; ++f) { a.packed[i * 4 + f] = word[f]; }
	a.packed[i * 4 + 3] = m;
}

__global__ __launch_bounds__(kThreads) void k_feat_fpfh(FeatArgs a)
{
	const int64_t r = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (r >= a.nf) { return; }
	const int64_t i = a.who[r];
	if (!a.live[i]) { return; }
	const unsigned long long mi = a.packed[i * 4 + 3];
	if (mi == 0) { return; }  // (zeros and valid = 0 stay)
	double pi[3];
	load3(a.pos, i, pi);
	double A[kWidth];
#pragma unroll
	for (int b = 0; b < kWidth; ++b) { A[b] = 0.0; }
	long q = 0;
	for (int e = 0; e < a.k; ++e) {
		const long long j = a.idx[r * a.k + e];
		double          dp[3], w;
		if (!neighbour(a, i, j, pi, dp, w)) { continue; }
		const unsigned long long mj = a.packed[j * 4 + 3];
		if (mj == 0) { continue; }
		const double count = static_cast<double>(mj);
#pragma unroll
		for (int f = 0; f < 3; ++f) {
			const unsigned long long word = a.packed[j * 4 + f];
			const bool               over = carried(word, mj);
#pragma unroll
			for (int b = 0; b < kBins; ++b) {
				const double c    = count_of(word, b, over);
				const double S    = (100.0 * c) / count;
				A[f * kBins + b] = A[f * kBins + b] + S / w;
			}
		}
		q += 1;
	}
	const double count = static_cast<double>(mi), share = static_cast<double>(q);
#pragma unroll
	for (int f = 0; f < 3; ++f) {
		const unsigned long long word = a.packed[i * 4 + f];
		const bool               over = carried(word, mi);
		double                   z    = 0.0;
#pragma unroll
		for (int b = 0; b < kBins; ++b) {
			const double c   = count_of(word, b, over);
			const double S   = (100.0 * c) / count;
			A[f * kBins + b] = S + (q > 0 ? A[f * kBins + b] / share : 0.0);
			z                = z + A[f * kBins + b];
		}
#pragma unroll
		for (int b = 0; b < kBins; ++b) {
			const double F                       = z > 0.0 ? (100.0 * A[f * kBins + b]) / z : A[f * kBins + b];
			a.features[i * kWidth + f * kBins + b] = static_cast<float>(F);
		}
	}
	if (a.valid) { a.valid[i] = 1; }
}

// ---- matching -----------------------------------------------------------------------------------------------------------

constexpr unsigned long long kNoMatch = ~0ull;

struct MatchArgs {
	int                  dim;
	int64_t              na, nb;
	const float*         a;
	const float*         b;
	const unsigned char* va;  // or null
	const unsigned char* vb;  // or null
	unsigned long long*  best; // [na]
};

// lane t of the workgroup owns row blockIdx.x * 256 + t of a, padded with zeros to DP columns: (0 - 0)^2 adds +0.0f, which
// changes no sum.  The workgroup walks the tiles blockIdx.y, blockIdx.y + gridDim.y, ... of b, so a lane meets its j ascending.
template <int DP>
__global__ __launch_bounds__(kThreads) void k_feat_match(MatchArgs g)
{
	__shared__ float s[kTile][DP];
	const int        t   = threadIdx.x;
	const int64_t    row = static_cast<int64_t>(blockIdx.x) * kThreads + t;
	float            x[DP];
#pragma unroll
	for (int c = 0; c < DP; ++c) { x[c] = row < g.na && c < g.dim ? g.a[row * g.dim + c] : 0.0f; }
	float    bs   = 0.0f;
	uint32_t bj   = kNone;
	for (int c = g.dim; c < DP; ++c) { s[t][c] = 0.0f; }  // (the padding columns, once: the staging leaves them alone)
	for (int64_t base = static_cast<int64_t>(blockIdx.y) * kTile; base < g.nb; base += static_cast<int64_t>(gridDim.y) * kTile) {
		__syncthreads();  // (the previous tile has been read)
		// the tile's rows lie one after the other in b: consecutive lanes copy consecutive floats
		const int have = static_cast<int>(g.nb - base < kTile ? g.nb - base : kTile) * g.dim;
		for (int at = t; at < have; at += kThreads) { s[at / g.dim][at % g.dim] = g.b[base * g.dim + at]; }
		__syncthreads();
		// a masked or non-finite row and a row past the end: one NaN makes every sum with it a NaN
		const int64_t j  = base + t;
		bool          ok = j < g.nb && (!g.vb || g.vb[j] != 0);
		if (ok) {
			for (int c = 0; c < g.dim; ++c) { ok = ok && isfinite(s[t][c]); }
		}
		if (!ok) { s[t][0] = NAN; }
		__syncthreads();
#pragma unroll 2
		for (int k = 0; k < kTile; ++k) {
			float sum = 0.0f;
#pragma unroll
			for (int c = 0; c < DP; ++c) {
				const float d = x[c] - s[k][c];
				sum           = sum + d * d;
			}
			// (a NaN compares false both times; +inf is admissible and wins only over nothing)
			if (sum < bs || (bj == kNone && sum == sum)) {
				bs = sum;
				bj = static_cast<uint32_t>(base + k);
			}
		}
	}
	if (row < g.na && bj != kNone) {
		atomicMin(&g.best[row], (static_cast<unsigned long long>(__float_as_uint(bs)) << 32) | bj);
	}
}

__global__ __launch_bounds__(kThreads) void k_feat_match_out(MatchArgs g, long long* __restrict__ indices, float* __restrict__ distances)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= g.na) { return; }
	bool ok = !g.va || g.va[i] != 0;
	for (int c = 0; c < g.dim; ++c) { ok = ok && isfinite(g.a[i * g.dim + c]); }
	const unsigned long long w = g.best[i];
	ok                         = ok && w != kNoMatch;
	indices[i]                 = ok ? static_cast<long long>(w & 0xFFFFFFFFull) : -1LL;
	if (distances) { distances[i] = ok ? sqrtf(__uint_as_float(static_cast<uint32_t>(w >> 32))) : INFINITY; }
}

template <int DP>
void launch_match(const MatchArgs& g, dim3 grid, hipStream_t st)
{
	hipLaunchKernelGGL(k_feat_match<DP>, grid, dim3(kThreads), 0, st, g);
}

}  // namespace

void points_describe(const NearestIndex& t, const float* normals, int k, float max_distance, float* features, unsigned char* valid,
                     int memory, hipStream_t st)
{
	const int64_t n = t.n, nf = t.nf;
	if (n == 0) { return; }
	AllocStream alloc_on(st);
	FeatArgs    a{};
	DevBuf      block;
	float *     pos = nullptr, *queries = nullptr, *dist = nullptr, *feat = nullptr;
	uint32_t*   who = nullptr;
	long long*  idx = nullptr;
	unsigned char* val = nullptr;
	arena_alloc(block, [&](Arena& ar) {
		a.unit   = ar.take<double>(n * 3);
		a.packed = ar.take<unsigned long long>(n * 4);
		idx      = ar.take<long long>(nf * k);
		pos      = ar.take<float>(n * 3);
		queries  = ar.take<float>(nf * 3);
		dist     = ar.take<float>(nf * k);
		who      = ar.take<uint32_t>(nf);
		a.normals = stage::in(ar, normals, n * 3, memory, st);
		feat     = stage::out(ar, features, n * kWidth, memory);
		a.live   = ar.take<unsigned char>(n);
		val      = stage::out(ar, valid, n, memory);
	});
	FI_HIP_TRY(hipMemsetAsync(pos, 0xFF, sizeof(float) * 3 * n, st));  // NaN
	FI_HIP_TRY(hipMemsetAsync(a.packed, 0, sizeof(unsigned long long) * 4 * n, st));
	FI_HIP_TRY(hipMemsetAsync(feat, 0, sizeof(float) * kWidth * n, st));
	if (val) { FI_HIP_TRY(hipMemsetAsync(val, 0, n, st)); }
	a.n        = n;
	a.nf       = nf;
	a.k        = k;
	a.who      = who;
	a.idx      = idx;
	a.pos      = pos;
	a.features = feat;
	a.valid    = val;
	const dim3 block_dim(kThreads);
	if (nf > 0) {
		hipLaunchKernelGGL(k_feat_positions, dim3(blocks_for(nf)), block_dim, 0, st, tree_of(t), pos, queries, who);
		FI_HIP_TRY(hipGetLastError());
		knn_query(t, nf, queries, k, max_distance, dist, idx, FI_DEVICE, st);
	}
	hipLaunchKernelGGL(k_feat_live, dim3(blocks_for(n)), block_dim, 0, st, a);
	if (nf > 0) {
		hipLaunchKernelGGL(k_feat_spfh, dim3(blocks_for(nf)), block_dim, 0, st, a);
		hipLaunchKernelGGL(k_feat_fpfh, dim3(blocks_for(nf)), block_dim, 0, st, a);
	}
	FI_HIP_TRY(hipGetLastError());
	stage::back(features, feat, n * kWidth, memory, st);
	stage::back(valid, val, n, memory, st);
	FI_HIP_TRY(hipStreamSynchronize(st));  // the temporaries die here
}

void feature_match(int dim, int64_t n_a, const float* a, const unsigned char* valid_a, int64_t n_b, const float* b,
                   const unsigned char* valid_b, long long* indices, float* distances, int memory)
{
	if (n_a == 0) { return; }
	hipStream_t st   = nullptr;
	MatchArgs   g{};
	DevBuf      block;
	float*      dd = nullptr;
	long long*  di = nullptr;
	arena_alloc(block, [&](Arena& ar) {  // (an empty b is not uploaded)
		g.best = ar.take<unsigned long long>(n_a);
		di     = stage::out(ar, indices, n_a, memory);
		g.a    = stage::in(ar, a, n_a * dim, memory, st);
		g.b    = stage::in(ar, b, n_b * dim, memory, st);
		dd     = stage::out(ar, distances, n_a, memory);
		g.va   = stage::in(ar, valid_a, n_a, memory, st);
		g.vb   = stage::in(ar, valid_b, n_b, memory, st);
	});
	FI_HIP_TRY(hipMemsetAsync(g.best, 0xFF, sizeof(unsigned long long) * n_a, st));  // kNoMatch
	g.dim = dim;
	g.na  = n_a;
	g.nb  = n_b;
	if (n_b > 0) {
		// about 2048 workgroups: the rows of a first, then as many chunks of b as that leaves room for
		const int64_t rows = blocks_for(n_a), tiles = (n_b + kTile - 1) / kTile;
		const dim3    grid(static_cast<unsigned>(rows), static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(tiles, 2048 / rows))));
		if (dim <= 8) {
			launch_match<8>(g, grid, st);
		} else if (dim <= 16) {
			launch_match<16>(g, grid, st);
		} else if (dim <= 32) {
			launch_match<32>(g, grid, st);
		} else if (dim <= 40) {
			launch_match<40>(g, grid, st);
		} else {
			launch_match<64>(g, grid, st);
		}
	}
	hipLaunchKernelGGL(k_feat_match_out, dim3(blocks_for(n_a)), dim3(kThreads), 0, st, g, di, dd);
	FI_HIP_TRY(hipGetLastError());
	stage::back(indices, di, n_a, memory, st);
	stage::back(distances, dd, n_a, memory, st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

}  // namespace fi
