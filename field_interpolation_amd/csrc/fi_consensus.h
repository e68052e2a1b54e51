// fi_consensus.h -- what a RANSAC unit is apart from its model (fi_plane.hip and fi_align.hip are its users):
// hypothesis h draws S of the `live` candidates by fi_uniform.h's counter hash; a batch of hypotheses is scored with integer
// counts; the best is the largest key count << 32 | (0xFFFFFFFF - h), so a tie goes to the lowest h, kept as one 64-bit
// maximum on the device; the host reads 16 bytes once a batch and asks the stop rule.  The model, its score kernel, the
// flags and the refits are the unit's own.
#pragma once

#include <algorithm>

#include "fi_internal.h"
#include "fi_uniform.h"

namespace fi {
namespace consensus {

// the start of a unit's device state: what the host reads once a batch
struct Head {
	unsigned long long best;   // the largest key so far (0: no valid hypothesis yet)
	uint32_t           live;   // the candidates the hypotheses draw from (select_indices writes it)
	uint32_t           spare;  // the unit's own word of a batch; the batch loop adds it up
};
static_assert(sizeof(Head) == 16, "one read-back of 16 bytes a batch");

__device__ inline unsigned long long key_of(uint32_t count, uint32_t h) { return (static_cast<unsigned long long>(count) << 32) | (0xFFFFFFFFu - h); }
inline uint64_t winner_of(unsigned long long key) { return 0xFFFFFFFFu - static_cast<uint32_t>(key & 0xFFFFFFFFull); }  // its h

// the body of a keys kernel, thread t over the slots of a batch that begins at hypothesis `first`: the key of a valid slot,
// the maximum of a wave by shuffles, one 64-bit integer atomic a wave; the counts are left zero
__device__ inline void keep_best(int t, int64_t first, const unsigned char* __restrict__ valid, uint32_t* __restrict__ counts, Head* head)
{
	unsigned long long key = valid[t] ? key_of(counts[t], static_cast<uint32_t>(first + t)) : 0ull;
	counts[t]              = 0;
	for (int o = 32; o > 0; o >>= 1) {
		const unsigned long long other = __shfl_xor(key, o, 64);
		key                            = other > key ? other : key;
	}
	if ((threadIdx.x & 63) == 0 && key != 0) { atomicMax(&head->best, key); }
}

// the S list positions of hypothesis h over live >= S candidates: j_k = min(floor(u(seed, h S + k) live), live - 1); false
// when two of them are the same
template <int S>
__device__ inline bool draw(uint64_t seed, uint64_t h, uint32_t live, uint32_t (&j)[S])
{
	bool distinct = true;
#pragma unroll
	for (int k = 0; k < S; ++k) {
		const double   u  = counter::uniform(seed, h * S + k);
		const uint64_t at = static_cast<uint64_t>(floor(u * static_cast<double>(live)));
		j[k]              = at < live - 1 ? static_cast<uint32_t>(at) : live - 1;
#pragma unroll
		for (int q = 0; q < k; ++q) { distinct = distinct && j[q] != j[k]; }
	}
	return distinct;
}

// the stop rule: r = (1 - w^S)^T by binary exponentiation from the low bit, w = b / live; add, multiply and compare only
inline bool confident(long long b, long long live, long long T, int S, double confidence)
{
	const double w = static_cast<double>(b) / static_cast<double>(live);
	double       p = w;
	for (int s = 1; s < S; ++s) { p = p * w; }
	double r = 1.0, base = 1.0 - p;
	for (unsigned long long e = static_cast<unsigned long long>(T); e; e >>= 1) {
		if (e & 1) { r = r * base; }
		base = base * base;
	}
	return r <= 1.0 - confidence;
}

struct Trials {
	Head      seen;   // the head as last read (best == 0: nothing was found)
	long long T;      // the hypotheses drawn
	long long spare;  // the spare word added over the batches
};

// enqueue(first, count) puts one batch on st: hypotheses first .. first + count - 1, and a keys kernel at its end.  After each
// the head is read; the loop leaves when fewer than S candidates are live (T stays 0), when max_trials are drawn, or when the
// stop rule says so.
template <class Enqueue>
inline Trials run_batches(const Head* head, int S, int batch, long long max_trials, double confidence, hipStream_t st, Enqueue&& enqueue)
{
	Trials r{};
	for (int64_t first = 0; first < max_trials; first += batch) {
		const int count = static_cast<int>(std::min<int64_t>(batch, max_trials - first));
		enqueue(first, count);
		FI_HIP_TRY(hipGetLastError());
		FI_HIP_TRY(hipMemcpyAsync(&r.seen, head, sizeof(Head), hipMemcpyDeviceToHost, st));
		FI_HIP_TRY(hipStreamSynchronize(st));
		if (r.seen.live < static_cast<uint32_t>(S)) { break; }
		r.T = first + count;
		r.spare += r.seen.spare;
		const long long b = static_cast<long long>(r.seen.best >> 32);
		if (b > 0 && confidence > 0.0 && confident(b, r.seen.live, r.T, S, confidence)) { break; }
	}
	return r;
}

}  // namespace consensus
}  // namespace fi
