// fi_surface.h -- exact distances to a segment (2-D) or triangle (3-D) mesh on the device, and the redistancing of a field
// against its own iso-surface (fi_surface.hip), shared by the C ABI unit (fi_capi.hip).
#pragma once

#include "fi_iso.h"

namespace fi {

// The search structure over one mesh: its usable primitives (every vertex coordinate finite) sorted by the Morton code of
// their box centres (over the mesh's own bounds), each stored with its vertex coordinates inline -- 3-D: three float4
// (a, b, c; the primitive's index as bits in the first .w), 2-D: one float4 (ax, ay, bx, by) and the index in `ids` -- under
// the tree of BvhIndex (fi_internal.h) with leaves of 8 primitives.
struct SurfaceIndex : BvhIndex {
	int     D  = 0;
	int64_t np = 0;   // primitives of the mesh (usable or not)
};

// a structure built from nv vertices (ndim floats each) and np primitives (ndim int32 indices each) already on the device;
// an index outside [0, nv): FI_ERR_INVALID
void surface_build(SurfaceIndex& t, int ndim, int64_t nv, const float* vertices, int64_t np, const int* indices, hipStream_t st);

// The queries of the C ABI (include/fi_hip.h fi_surface_distance): queries and outputs in `memory`; primitives and closest
// may be null.
void surface_query(const SurfaceIndex& t, int64_t n, const float* queries, float max_distance, float* distances,
                   long long* primitives, float* closest, int memory, hipStream_t st);
// every point of a lattice (x fastest) as a query, unsigned
void surface_lattice(const SurfaceIndex& t, const int* sizes, float max_distance, float* out, long long* primitives, int memory,
                     hipStream_t st);

// fi_redistance_field on a whole fp32 field already on the device; out / primitives in `memory`; mesh: null, or receives
// the mesh the primitive indices refer to
void redistance_whole(const float* field, int ndim, const int* sizes, float iso, int method, float max_distance, float* out,
                      long long* primitives, fi_mesh** mesh, int memory, hipStream_t st);
// fi_redistance: an undivided context's field (memory: FI_HOST / FI_DEVICE) or, with nullptr, its last solution
void redistance_ctx(fi_ctx* c, const float* field, float iso, int method, float max_distance, float* out, long long* primitives,
                    fi_mesh** mesh, int memory);

}  // namespace fi

// a mesh of its own (fi_surface_create, include/fi_hip.h): its search structure on the device it was created on
struct fi_surface {
	int                device = 0;
	fi::SurfaceIndex   t;
};
