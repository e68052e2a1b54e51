// fi_knn_list.h -- the register-resident list of the k best pairs that the units walking fi_nearest.h's tree for more than one
// neighbour share (fi_knn.hip: queries and normals; fi_cloud.hip: the neighbour distances of a set's own points).  The list
// code is fi_knn.hip's, moved here as it was.
#pragma once

#include "fi_solver_internal.h"
#include "fi_nearest.h"
#include "fi_bvh.h"

namespace fi {
namespace knn {

using bvh::kNone;

__device__ inline bool pair_less(float s, uint32_t j, float s1, uint32_t j1) { return s < s1 || (s == s1 && j < j1); }

// The k best pairs (s, j) in ascending order as entries [CAP - k, CAP) of a list of CAP entries, each with its sorted slot of
// the tree (`at`: dead code where nobody reads it).  The list is a chain of structs walked by template recursion, entry
// N - 1 last: every access names its entry at compile time, so the whole list lives in registers.
template <int N>
struct List {
	List<N - 1> lo;  // the entries before this one
	float       s;
	uint32_t    j, at;
};
template <>
struct List<0> {};

// entries [first_open, CAP) empty (+inf, no index); those in front blocked: (-1, 0) sorts before every pair, so a blocked
// entry is never displaced and never shifted
template <int N>
__device__ __forceinline__ void list_reset(List<N>& l, int first_open)
{
	if constexpr (N > 0) {
		const bool open = N - 1 >= first_open;
		l.s  = open ? INFINITY : -1.0f;
		l.j  = open ? kNone : 0u;
		l.at = 0u;
		list_reset<N - 1>(l.lo, first_open);
	}
}

// the pair sorts before entry N - 1: that entry's predecessor moves up into it while the pair sorts before that one as
// well, else the pair lands here (the old entry N - 1 has gone to N, or is dropped at the end of the list)
template <int N>
__device__ __forceinline__ void list_put(List<N>& l, float ns, uint32_t nj, uint32_t slot)
{
	if constexpr (N == 1) {
		l.s  = ns;
		l.j  = nj;
		l.at = slot;
	} else {
		const bool up = pair_less(ns, nj, l.lo.s, l.lo.j);
		l.s  = up ? l.lo.s : ns;
		l.j  = up ? l.lo.j : nj;
		l.at = up ? l.lo.at : slot;
		if (up) { list_put<N - 1>(l.lo, ns, nj, slot); }
	}
}

// accept a pair only if it sorts before the k-th
template <int N>
__device__ __forceinline__ void list_offer(List<N>& l, float ns, uint32_t nj, uint32_t slot)
{
	if (pair_less(ns, nj, l.s, l.j)) { list_put<N>(l, ns, nj, slot); }
}

// f(r, s, j, at) for every entry in ascending order
template <int N, class F>
__device__ __forceinline__ void list_each(const List<N>& l, F&& f)
{
	if constexpr (N > 0) {
		list_each<N - 1>(l.lo, f);
		f(N - 1, l.s, l.j, l.at);
	}
}

// a pair found (as opposed to a blocked or an empty entry) within lim
__device__ inline bool found(float s, uint32_t j, float lim) { return s >= 0.0f && j != kNone && !(s > lim); }

// the list's capacity class of a k
inline int capacity_for(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : 32; }

}  // namespace knn
}  // namespace fi
