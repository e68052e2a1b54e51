// fi_prim.h -- the device-wide primitives of the assembly (scans, run-length encoding, selection, 64-bit
// pair sorts) straight on rocPRIM, ROCm's own primitive library (rounds 1-4 went through hipCUB, the CUB-shaped layer over
// it).  Same call shape as the library's: a first call with a null workspace returns the bytes it wants.  Below them the
// host side the units share: a call's temporaries as pieces of one block, the size-then-run pairs (sorts, scans, selections).
#pragma once

#include <cstring>
#include <iterator>

#include <rocprim/rocprim.hpp>

#include "fi_arena.h"
#include "fi_internal.h"

namespace fi {
namespace prim {

template <typename In, typename Out>
inline hipError_t exclusive_sum(void* tmp, size_t& bytes, In in, Out out, size_t n, hipStream_t st)
{
	using T = typename std::iterator_traits<Out>::value_type;
	return rocprim::exclusive_scan(tmp, bytes, in, out, T(0), n, rocprim::plus<T>(), st);
}

// runs of equal keys: the distinct keys, the run lengths, the number of runs
template <typename In, typename Unique, typename Counts, typename Runs>
inline hipError_t run_length_encode(void* tmp, size_t& bytes, In in, Unique unique_out, Counts counts_out, Runs runs_out, size_t n,
                                    hipStream_t st)
{
	return rocprim::run_length_encode(tmp, bytes, in, static_cast<unsigned int>(n), unique_out, counts_out, runs_out, st);
}

// out = the indices 0 .. n-1 the predicate accepts, in order; *count_out = how many
template <typename Out, typename Count, typename Pred>
inline hipError_t select_indices(void* tmp, size_t& bytes, Out out, Count count_out, size_t n, Pred pred, hipStream_t st)
{
	return rocprim::select(tmp, bytes, rocprim::counting_iterator<uint32_t>(0u), out, count_out, n, pred, st);
}

// stable radix sort of (key, value) pairs over key bits [begin_bit, end_bit); 64-bit keys: Onesweep with the workgroup shape
// tuned for the 32-bit sorts of fi_sort.h (1024 threads x 8 items; the library's default merge-sorts below 2^20 items: a dozen
// pairs of small launches where Onesweep takes one histogram, one scan and a pass per digit)
namespace detail {
using onesweep64 = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                              rocprim::radix_sort_onesweep_config<rocprim::kernel_config<1024, 8>, rocprim::kernel_config<1024, 8>, 8,
                                                                                  rocprim::block_radix_rank_algorithm::match>,
                                              16384>;
}
template <typename V>
inline hipError_t sort_pairs_u64(void* tmp, size_t& bytes, const uint64_t* keys_in, uint64_t* keys_out, const V* values_in, V* values_out,
                                 size_t n, int begin_bit, int end_bit, hipStream_t st)
{
	return rocprim::radix_sort_pairs<detail::onesweep64>(tmp, bytes, keys_in, keys_out, values_in, values_out, static_cast<unsigned int>(n),
	                                                     static_cast<unsigned int>(begin_bit), static_cast<unsigned int>(end_bit), st);
}

// the same sort of bare keys (fi_smooth.hip's directed vertex pairs: the key is all there is)
inline hipError_t sort_keys_u64(void* tmp, size_t& bytes, const uint64_t* keys_in, uint64_t* keys_out, size_t n, int begin_bit, int end_bit,
                                hipStream_t st)
{
	return rocprim::radix_sort_keys<detail::onesweep64>(tmp, bytes, keys_in, keys_out, static_cast<unsigned int>(n),
	                                                    static_cast<unsigned int>(begin_bit), static_cast<unsigned int>(end_bit), st);
}

// ---- the host side of a unit built on these: one arena (fi_arena.h) for a call's temporaries, a piece of it as workspace ---

// the primitives' workspace: a piece of the arena sized (scan_bytes, sort_bytes) for the call's largest sort and scan
struct Scratch {
	void*  p     = nullptr;
	size_t bytes = 0;
};

// lay_out(arena) takes a call's pieces: run once for their size, then over `block` allocated to that size
template <class F>
inline void arena_alloc(DevBuf& block, F&& lay_out)
{
	Arena sizing(nullptr);
	lay_out(sizing);
	block.alloc(sizing.bytes());
	Arena arena(block.p);
	lay_out(arena);
}

// the run of a size-then-run pair: call(workspace, bytes) is asked with a null workspace, then run in tmp -- or in a block of
// its own, should the library want more for fewer items or bits than the sizing pass asked about
template <class Call>
inline void run_in(const Scratch& tmp, Call&& call)
{
	size_t tb = 0;
	FI_HIP_TRY(call(nullptr, tb));
	DevBuf more;
	if (tb > tmp.bytes) { more.alloc(tb); }
	FI_HIP_TRY(call(more.p ? more.p : tmp.p, tb));
}

template <typename Out = uint32_t>
inline size_t scan_bytes(int64_t n)
{
	size_t tb = 0;
	FI_HIP_TRY(exclusive_sum(nullptr, tb, static_cast<const uint32_t*>(nullptr), static_cast<Out*>(nullptr), static_cast<size_t>(n), nullptr));
	return tb;
}

// out = the exclusive prefix sums of n uint32
template <typename Out>
inline void scan_u32(const uint32_t* in, Out* out, int64_t n, const Scratch& tmp, hipStream_t st)
{
	run_in(tmp, [&](void* p, size_t& tb) { return exclusive_sum(p, tb, in, out, static_cast<size_t>(n), st); });
}

// the same scan of n uint64 (fi_meshpts.hip's integer weights reach 2^32: one bit more than a uint32 holds)
inline size_t scan_u64_bytes(int64_t n)
{
	size_t tb = 0;
	FI_HIP_TRY(exclusive_sum(nullptr, tb, static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr), static_cast<size_t>(n), nullptr));
	return tb;
}

inline void scan_u64(const uint64_t* in, uint64_t* out, int64_t n, const Scratch& tmp, hipStream_t st)
{
	run_in(tmp, [&](void* p, size_t& tb) { return exclusive_sum(p, tb, in, out, static_cast<size_t>(n), st); });
}

template <typename V = uint32_t>
inline size_t sort_bytes(int64_t n, int begin_bit, int end_bit)
{
	size_t tb = 0;
	FI_HIP_TRY(sort_pairs_u64(nullptr, tb, static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr), static_cast<const V*>(nullptr),
	                          static_cast<V*>(nullptr), static_cast<size_t>(n), begin_bit, end_bit, nullptr));
	return tb;
}

// (kout, vout) = the pairs (kin, vin) in ascending order of key bits [begin_bit, end_bit), stable
template <typename V>
inline void sort_u64(const uint64_t* kin, uint64_t* kout, const V* vin, V* vout, int64_t n, int begin_bit, int end_bit, const Scratch& tmp,
                     hipStream_t st)
{
	run_in(tmp, [&](void* p, size_t& tb) { return sort_pairs_u64(p, tb, kin, kout, vin, vout, static_cast<size_t>(n), begin_bit, end_bit, st); });
}

inline size_t sort_keys_bytes(int64_t n, int begin_bit, int end_bit)
{
	size_t tb = 0;
	FI_HIP_TRY(sort_keys_u64(nullptr, tb, static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr), static_cast<size_t>(n), begin_bit,
	                         end_bit, nullptr));
	return tb;
}

// kout = the keys kin in ascending order of bits [begin_bit, end_bit)
inline void sort_keys(const uint64_t* kin, uint64_t* kout, int64_t n, int begin_bit, int end_bit, const Scratch& tmp, hipStream_t st)
{
	run_in(tmp, [&](void* p, size_t& tb) { return sort_keys_u64(p, tb, kin, kout, static_cast<size_t>(n), begin_bit, end_bit, st); });
}

// a selection by flags: the predicate of select_indices over uint8 marks
struct Marked {
	const unsigned char* f;
	__device__ bool      operator()(uint32_t i) const { return f[i] != 0; }
};

inline size_t select_bytes(int64_t n)
{
	size_t tb = 0;
	FI_HIP_TRY(select_indices(nullptr, tb, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<size_t>(n), Marked{nullptr},
	                          nullptr));
	return tb;
}

// out = the indices i < n with f[i] != 0, ascending; *count = how many
inline void select_marked(const unsigned char* f, uint32_t* out, uint32_t* count, int64_t n, const Scratch& tmp, hipStream_t st)
{
	run_in(tmp, [&](void* p, size_t& tb) { return select_indices(p, tb, out, count, static_cast<size_t>(n), Marked{f}, st); });
}

inline uint32_t read_u32(const uint32_t* dev, hipStream_t st)
{
	uint32_t h = 0;
	FI_HIP_TRY(hipMemcpyAsync(&h, dev, sizeof(h), hipMemcpyDeviceToHost, st));
	FI_HIP_TRY(hipStreamSynchronize(st));
	return h;
}

inline int bits_for(int64_t count)  // key bits that tell `count` values apart (at least one)
{
	int b = 1;
	while ((int64_t(1) << b) < count) { ++b; }
	return b;
}

// one thread per item in work groups of kGridThreads (the kThreads of the units that launch with it), at least one group
constexpr int kGridThreads = 256;
inline dim3   grid(int64_t n) { return dim3(static_cast<unsigned>(((n > 0 ? n : 1) + kGridThreads - 1) / kGridThreads)); }

}  // namespace prim
}  // namespace fi
