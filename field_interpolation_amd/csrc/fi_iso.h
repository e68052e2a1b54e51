// fi_iso.h -- iso-contour / iso-surface extraction (fi_iso.hip), shared by the C ABI units (fi_capi.hip, fi_group.hip).
#pragma once

#include "fi_internal.h"

// the device-resident mesh of fi_iso_extract* (include/fi_hip.h)
struct fi_mesh {
	int        device = 0;
	int        ndim = 0;
	int64_t    nv = 0, np = 0;   // vertices, primitives (segments in 2-D, triangles in 3-D)
	fi::DevBuf pos, nrm;         // float[nv][ndim]
	fi::DevBuf idx;              // int32[np][ndim]
	fi::DevBuf key;              // int64[nv], ascending
};

namespace fi {

// A whole field on the device (float, x fastest).  `pieces` meshes: piece r holds the cells whose slowest coordinate lies in
// the equal slab split's [lo_r, hi_r) (fi_slab_partition), with every vertex they use; pieces == 1: the undivided mesh.
void iso_extract_whole(const float* field, int ndim, const int* sizes, float iso, int pieces, const int* slab_lo,
                       const int* slab_hi, hipStream_t st, fi_mesh** out);
// The piece of a slab context (nranks > 1, its own transport) or the mesh of an undivided one.  field: the context's owned
// values (memory: FI_HOST / FI_DEVICE) or nullptr for the last solution.
void iso_extract_ctx(fi_ctx* c, const float* field, float iso, int memory, fi_mesh** out);
// a loop-back group's members, in rank order.  whole: the undivided field on the host (each piece reads its window of it),
// or nullptr: the members' last solutions, through the same ghost-plane exchange as iso_extract_ctx's slab contexts
void iso_extract_group(std::vector<fi_ctx*>& members, const float* whole, float iso, fi_mesh** out);

}  // namespace fi
