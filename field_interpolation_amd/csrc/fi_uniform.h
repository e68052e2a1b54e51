// fi_uniform.h -- the counter-based uniform number of the sampling units: fi_meshpts.hip (a sample's stratum and its place in
// the primitive) and fi_plane.hip (the points a hypothesis draws).  splitmix64's finaliser over seed + (counter + 1) golden,
// the top 53 bits as a double in [0, 1): a draw is a function of (seed, counter) alone, whatever thread computes it.
// tests/meshpts_reference.py's uniform() is the same arithmetic in numpy.
//
// A device inline: both units include it.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace fi {
namespace counter {

__device__ inline double uniform(uint64_t seed, uint64_t counter)
{
	uint64_t z = seed + (counter + 1) * 0x9E3779B97F4A7C15ull;
	z ^= z >> 30;
	z *= 0xBF58476D1CE4E5B9ull;
	z ^= z >> 27;
	z *= 0x94D049BB133111EBull;
	z ^= z >> 31;
	return static_cast<double>(z >> 11) * 0x1.0p-53;
}

}  // namespace counter
}  // namespace fi
