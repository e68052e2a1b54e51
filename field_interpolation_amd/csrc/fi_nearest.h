// fi_nearest.h -- exact nearest data points on the device (fi_nearest.hip), shared by the C ABI unit (fi_capi.hip) and the
// border prior (fi_assembly.hip).
#pragma once

#include "fi_internal.h"

namespace fi {

// The search structure over one point set: the finite points sorted by their Morton code (over their own bounding box),
// float4 each (x, y, z, the point's index as bits), under the tree of BvhIndex (fi_internal.h) with leaves of 16 points.
struct NearestIndex : BvhIndex {
	int     D = 0;
	int64_t n = 0;   // points of the set (finite or not)
	DevBuf  rest;    // the n - nf points left out of the tree, in no order: float4 each (x, y, z, the index as bits) -- what a
	                 // unit that hands a set's own points back (fi_mls.hip) returns for them
};

// what the units that walk this tree share (fi_nearest.hip, fi_knn.hip): the points of a leaf ...
constexpr int kNearestLeaf = 16;

// ... and s(p, q) of the contract for a stored point p and a query q
template <int D>
__device__ inline float sq_dist(const float4& p, const float* q)
{
	const float c[3] = {p.x, p.y, p.z};
	float       s    = 0.0f;
#pragma unroll
	for (int d = 0; d < D; ++d) {
		const float e = c[d] - q[d];
		s = s + e * e;
	}
	return s;
}

// the set of a context: its fi_add_points batches in call order, the border prior's left out (PointBatch::prior); built on
// the context's stream, kept in c->nearest until the next fi_add_points / fi_clear_points
const NearestIndex& nearest_of(fi_ctx* c);
void                nearest_release(fi_ctx* c);
// a set built from n positions of ndim floats already on the device
void nearest_build(NearestIndex& t, int ndim, int64_t n, const float* const* seg_pos, const int64_t* seg_n, int nseg, hipStream_t st);

// The queries of the C ABI (include/fi_hip.h fi_nearest): queries / distances / indices in `memory`; indices may be null.
void nearest_query(const NearestIndex& t, int64_t n, const float* queries, float max_distance, float* distances,
                   long long* indices, int memory, hipStream_t st);
// every point of a lattice (x fastest) as a query
void nearest_lattice(const NearestIndex& t, const int* sizes, float max_distance, float* distances, long long* indices, int memory,
                     hipStream_t st);
// the border prior: the lattice points idx[0 .. nb) (linear indices of the lattice n[0 .. D)) as queries; d2 receives the
// SQUARED distance (the minimum of s, +inf with no finite point) on the device, enqueued on st
void nearest_lattice_list_d2(const NearestIndex& t, const int* n, int64_t nb, const uint32_t* idx, float* d2, hipStream_t st);

}  // namespace fi

// a point set of its own (fi_points_create, include/fi_hip.h): its search structure on the device it was created on
struct fi_points {
	int              device = 0;
	fi::NearestIndex t;
};
