// fi_sample.h -- point queries of a lattice field (fi_sample.hip), shared by the C ABI units (fi_capi.hip, fi_group.hip).
#pragma once

#include "fi_internal.h"

namespace fi {

// A whole field (float, x fastest; memory: FI_HOST / FI_DEVICE, as every other buffer of the call) at n positions.
void sample_field(const float* field, int ndim, const int* sizes, int64_t n, const float* positions, int mode, float fill,
                  float* values, float* gradients, int memory);
// A context's field: its owned values (fp32) or, field == nullptr, its last solution where it lives.  A slab context
// (nranks > 1, its own transport) samples the points whose cell lies in its slab and sums the results over the ranks.
void sample_ctx(fi_ctx* c, const float* field, int64_t n, const float* positions, int mode, float fill, float* values,
                float* gradients, int memory);
// a loop-back group's members, in rank order; whole: the undivided field on the host, or nullptr for the members' last
// solutions.  Every buffer on the host.
void sample_group(std::vector<fi_ctx*>& members, const float* whole, int64_t n, const float* positions, int mode, float fill,
                  float* values, float* gradients);

}  // namespace fi
