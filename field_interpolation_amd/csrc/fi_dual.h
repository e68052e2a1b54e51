// fi_dual.h -- dual contouring of a lattice field (fi_dual.hip), shared by the C ABI unit (fi_capi.hip).
#pragma once

#include "fi_iso.h"

namespace fi {

// A whole field on the device (float, x fastest) and, optionally, its gradients on the device (ndim floats per point,
// interleaved; nullptr: central differences of f - iso).  One undivided mesh (include/fi_hip.h fi_dual_contour).
void dual_contour_whole(const float* field, const float* gradients, int ndim, const int* sizes, float iso, hipStream_t st,
                        fi_mesh** out);
// An undivided context: field = its owned values (memory: FI_HOST / FI_DEVICE) or nullptr for the last solution; gradients in
// the same memory, or nullptr.  Slab contexts: FI_ERR_UNSUPPORTED.
void dual_contour_ctx(fi_ctx* c, const float* field, const float* gradients, float iso, int memory, fi_mesh** out);

}  // namespace fi
