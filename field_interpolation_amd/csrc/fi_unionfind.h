// fi_unionfind.h -- the lock-free union-find of the labelling units: fi_parts.hip (the vertices of a mesh, joined by its
// primitives) and fi_cluster.hip (the core points of a cloud, joined by the pairs within eps).  One 32-bit parent word per
// element.  Every union hooks the LARGER root under the smaller by a compare-and-swap on that root's own word: a parent
// never exceeds its child, so the forest has no cycle and a set's root is its smallest element whatever the timing.  A failed
// swap means another thread's swap on that word succeeded; the loser finds again -- no thread waits for a value another
// workgroup has yet to write.  (fi_orient.hip's variant carries a parity along every path and stays in its unit.)
//
// Everything here is a device inline: both units include it.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace fi {
namespace unionfind {

__device__ inline uint32_t word_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void word_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of v's tree as it stands, halving the path on the way (every word written is an ancestor of its vertex)
__device__ inline uint32_t find_root(uint32_t* parent, uint32_t v)
{
	for (;;) {
		const uint32_t p = word_load(&parent[v]);
		if (p == v) { return v; }
		const uint32_t g = word_load(&parent[p]);
		if (g == p) { return p; }
		word_store(&parent[v], g);
		v = g;
	}
}

__device__ inline void unite(uint32_t* parent, uint32_t a, uint32_t b)
{
	for (;;) {
		a = find_root(parent, a);
		b = find_root(parent, b);
		if (a == b) { return; }
		const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
		const uint32_t was = atomicCAS(&parent[hi], hi, lo);
		if (was == hi) { return; }
		// hi is no root any more: somebody else's swap succeeded and hung it under `was`; that tree and lo's are still to be joined
		a = was;
		b = lo;
	}
}

}  // namespace unionfind
}  // namespace fi
