// fi_treesum.h -- the contract's fixed-order sum on the device (tests/meshpts_reference.py's tree_sum is
// its definition in numpy): the terms in blocks of 256 consecutive items, a block summed by the tree s[t] += s[t + w],
// w = 128 .. 1, a missing item adding 0.0; the block sums added from 0.0 in ascending block order.  Every rounding is fixed
// by the terms and their order alone, so the sum does not know the launch shape.
//
// Used by fi_plane.hip, fi_align.hip and fi_cloud.hip.  Left out on purpose -- their trees are other programs, and taking
// them in would make these functions branch on their caller:
//   fi_cluster.hip  folds min/max boxes and a core count in the same loop as the sums;
//   fi_parts.hip    sums per wave (wave_sum) and adds the four waves in wave order;
//   fi_register.hip runs the tree by shuffles below w = 64;
//   fi_meshpts.hip  packs its LDS and finishes with a single thread.
// The first two share only the integer functions at the end: a count of flags, and how groups of items are cut into chunks.
#pragma once

#include <hip/hip_runtime.h>

namespace fi {
namespace treesum {

constexpr int kChunk = 256;  // the contract's block: a workgroup of kChunk lanes, an item each

// the block tree over K sums carried together: lane t's terms go to s[k][t]; the sums are left in s[k][0].  Every lane of
// the workgroup calls it.
template <int K>
__device__ inline void block_tree(const double (&v)[K], double (&s)[K][kChunk])
{
	const int t = threadIdx.x;
#pragma unroll
	for (int k = 0; k < K; ++k) { s[k][t] = v[k]; }
	__syncthreads();
	for (int w = kChunk / 2; w > 0; w >>= 1) {
		if (t < w) {
#pragma unroll
			for (int k = 0; k < K; ++k) { s[k][t] = s[k][t] + s[k][t + w]; }
		}
		__syncthreads();
	}
}

// one wave: total[k] = the block sums partial[b * stride + k], b = 0 .. nb - 1, added in ascending order from 0.0 (64 blocks
// a load, handed to every lane in turn).  Every lane of the wave calls it and gets the totals.
template <int K>
__device__ inline void ordered_sum(const double* __restrict__ partial, int stride, int64_t nb, int lane, double (&total)[K])
{
#pragma unroll
	for (int k = 0; k < K; ++k) { total[k] = 0.0; }
	for (int64_t b0 = 0; b0 < nb; b0 += 64) {
		const bool have = b0 + lane < nb;
		double     v[K];
#pragma unroll
		for (int k = 0; k < K; ++k) { v[k] = have ? partial[(b0 + lane) * stride + k] : 0.0; }
		const int e = nb - b0 < 64 ? static_cast<int>(nb - b0) : 64;
		for (int l = 0; l < e; ++l) {
#pragma unroll
			for (int k = 0; k < K; ++k) { total[k] = total[k] + __shfl(v[k], l, 64); }
		}
	}
}

// ---- integers, which add up the same in any order ----------------------------------------------------------------------

// one add per wave of the lanes whose flag is set (every lane of the wave calls this)
__device__ inline void count_flags(bool flag, unsigned long long* total)
{
	const unsigned long long lanes = __ballot(flag);
	if ((threadIdx.x & 63) == 0 && lanes != 0) { atomicAdd(total, static_cast<unsigned long long>(__popcll(lanes))); }
}

// groups of sorted items cut into chunks (fi_cluster.hip's clusters, fi_parts.hip's parts): group c holds the sorted items
// first[c] .. first[c + 1]; nchunks, scanned, gives chunk_first.  Entry c of nchunks, c = 0 .. groups: the chunks of group c
// (entry `groups`: 0, the scan's total)
__device__ inline uint32_t chunks_of(const uint32_t* __restrict__ first, int64_t c, int64_t groups)
{
	return c < groups ? (first[c + 1] - first[c] + kChunk - 1) / kChunk : 0u;
}

// the group of a chunk: the last c with chunk_first[c] <= chunk (a group without items has no chunk and shares its entry
// with the next one)
__device__ inline int64_t owner_of(const uint32_t* __restrict__ chunk_first, int64_t groups, uint32_t chunk)
{
	int64_t lo = 0, hi = groups - 1;
	while (lo < hi) {
		const int64_t mid = (lo + hi + 1) / 2;
		if (chunk_first[mid] <= chunk) {
			lo = mid;
		} else {
			hi = mid - 1;
		}
	}
	return lo;
}

}  // namespace treesum
}  // namespace fi
