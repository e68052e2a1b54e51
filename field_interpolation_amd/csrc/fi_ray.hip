// fi_ray.hip -- rays against a segment (2-D) or triangle (3-D) mesh on the device: the closest hit, the number of hits, the
// parity of the hits (containment) and with it a sign for the exact distances of fi_surface.hip.
//
// The contract (include/fi_hip.h fi_surface_raycast; tests/ray_reference.py restates it in numpy): the
// projection of Woop, Benthin and Wald's watertight test in fp32 -- kz the axis of the largest |d|, kx and ky the next two,
// swapped when d[kz] < 0, Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]; per vertex p = v - o,
// X = p[kx] - Sx p[kz], Y = p[ky] - Sy p[kz], Z = Sz p[kz] -- then the edge functions U = Cx By - Cy Bx, V = Ax Cy - Ay Cx,
// W = Bx Ay - By Ax in fp64, where the products of fp32 values are exact and so are the sign and the zero of each
// difference.  A triangle is hit when U, V, W are all >= 0 or all <= 0, not all zero, and it owns every edge on which it is
// zero (rasterisation's fill rule: B->C belongs to U, C->A to V, A->B to W, the direction negated for the negative
// orientation; owned when dy > 0, or dy = 0 and dx < 0): a ray through a shared edge or vertex meets exactly one of the
// triangles around it on each sheet.  t = fp32(((U Az + V Bz) + W Cz) / ((U + V) + W)) clamped into [min Z, max Z] of the
// three vertices.  2-D: X and Z alone; a segment is crossed when (Xa > 0) != (Xb > 0), t = fp32(Za + s (Zb - Za)) with
// s = Xa / (Xa - Xb) in fp64, clamped into [min Z, max Z].  Everything is compiled with -ffp-contract=off.
//
// The walk needs no margin: every rounded operation above is monotone in each vertex coordinate, so the same fp32
// expressions at the corner of a node box chosen by the sign of Sx (Sy, Sz) bound the X (Y, Z) of every vertex inside, bit
// for bit.  A hit needs min X <= 0 <= max X, min Y <= 0 <= max Y and t inside the vertices' Z range, so a box with
// Xmin > 0, Xmax < 0 (the same in Y), Zmax < t_min or Zmin > min(best, t_max) holds no hit that matters.  Every test is a
// positive comparison: a NaN bound (inf - inf from an overflow) prunes nothing.  The walk itself is fi_bvh.h's: stackless in
// heap numbering, one bit per level, the child with the smaller Zmin first (a tie: the left one), one thread per ray, no
// atomics.  The axis permutation is picked with selects, never by indexing a register array at run time (scratch).
#include "fi_solver_internal.h"
#include "fi_ray.h"
#include "fi_bvh.h"

#include <climits>

namespace fi {

namespace {

using namespace bvh;

constexpr int kRayLeaf = 8;  // fi_surface.hip's leaves

__device__ inline float pick(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }
__device__ inline float pick(const float4& v, int k) { return pick(v.x, v.y, v.z, k); }

// a usable ray: its permutation, its shear and its origin in permuted order
struct Ray {
	int   kx, ky, kz;
	float ox, oy, oz;
	float Sx, Sy, Sz;
};

// false: a non-finite origin or direction, or d = 0
template <int D>
__device__ inline bool ray_setup(const float* o, const float* d, Ray& r)
{
	if (!finite_point<D>(o) || !finite_point<D>(d)) { return false; }
	const float o2 = D == 3 ? o[2] : 0.0f, d2 = D == 3 ? d[2] : 0.0f;
	const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d2);
	if (!(ax > 0.0f || ay > 0.0f || az > 0.0f)) { return false; }
	if constexpr (D == 3) {
		r.kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);  // the lowest axis on ties
		int kx = r.kz == 2 ? 0 : r.kz + 1, ky = kx == 2 ? 0 : kx + 1;
		if (pick(d[0], d[1], d2, r.kz) < 0.0f) {
			const int s = kx;
			kx = ky;
			ky = s;
		}
		r.kx = kx;
		r.ky = ky;
	} else {
		r.kz = ax >= ay ? 0 : 1;
		r.kx = 1 - r.kz;
		r.ky = r.kx;
	}
	const float dz = pick(d[0], d[1], d2, r.kz);
	r.Sx = pick(d[0], d[1], d2, r.kx) / dz;
	r.Sy = D == 3 ? pick(d[0], d[1], d2, r.ky) / dz : 0.0f;
	r.Sz = 1.0f / dz;
	r.ox = pick(o[0], o[1], o2, r.kx);
	r.oy = pick(o[0], o[1], o2, r.ky);
	r.oz = pick(o[0], o[1], o2, r.kz);
	return true;
}

// the projection of one vertex
template <int D>
__device__ inline void project(const Ray& r, float vx, float vy, float vz, float& X, float& Y, float& Z)
{
	const float pz = pick(vx, vy, vz, r.kz) - r.oz;
	X = (pick(vx, vy, vz, r.kx) - r.ox) - r.Sx * pz;
	if constexpr (D == 3) { Y = (pick(vx, vy, vz, r.ky) - r.oy) - r.Sy * pz; }
	Z = r.Sz * pz;
}

__device__ inline float clamp_into(float t, float lo, float hi) { return t < lo ? lo : (t > hi ? hi : t); }

// the edge from (x0, y0) to (x1, y1) is the triangle's: dy > 0, or dy = 0 and dx < 0, of the direction negated for !pos
__device__ inline bool owns(bool pos, float x0, float y0, float x1, float y1)
{
	const bool up = y1 > y0 || (y1 == y0 && x1 < x0), down = y1 < y0 || (y1 == y0 && x1 > x0);
	return pos ? up : down;
}

// sorted slot i against the ray: hit or not in [t_min, t_max], its t and its primitive index; BARY: the barycentrics too
template <int D, bool BARY>
__device__ inline bool primitive_hit(const Tree& tr, int64_t i, const Ray& r, float t_min, float t_max, float* t_out, uint32_t* j,
                                     float* bary)
{
	float t;
	bool  hit;
	if constexpr (D == 3) {
		const float4 r0 = tr.items[3 * i], r1 = tr.items[3 * i + 1], r2 = tr.items[3 * i + 2];
		*j = __float_as_uint(r0.w);
		float Ax, Ay, Az, Bx, By, Bz, Cx, Cy, Cz;
		project<3>(r, r0.x, r0.y, r0.z, Ax, Ay, Az);
		project<3>(r, r1.x, r1.y, r1.z, Bx, By, Bz);
		project<3>(r, r2.x, r2.y, r2.z, Cx, Cy, Cz);
		const double ax = Ax, ay = Ay, bx = Bx, by = By, cx = Cx, cy = Cy;
		const double U = cx * by - cy * bx;
		const double V = ax * cy - ay * cx;
		const double W = bx * ay - by * ax;
		const bool pos = U >= 0.0 && V >= 0.0 && W >= 0.0, neg = U <= 0.0 && V <= 0.0 && W <= 0.0;
		hit = (pos || neg) && !(U == 0.0 && V == 0.0 && W == 0.0);
		hit = hit && (U != 0.0 || owns(pos, Bx, By, Cx, Cy));
		hit = hit && (V != 0.0 || owns(pos, Cx, Cy, Ax, Ay));
		hit = hit && (W != 0.0 || owns(pos, Ax, Ay, Bx, By));
		if (!hit) { return false; }
		const double det = (U + V) + W;
		const double num = (U * static_cast<double>(Az) + V * static_cast<double>(Bz)) + W * static_cast<double>(Cz);
		t = clamp_into(static_cast<float>(num / det), fminf(fminf(Az, Bz), Cz), fmaxf(fmaxf(Az, Bz), Cz));
		if constexpr (BARY) {
			bary[0] = static_cast<float>(V / det);
			bary[1] = static_cast<float>(W / det);
		}
	} else {
		const float4 s = tr.items[i];
		*j = tr.ids[i];
		float Xa, Xb, Za, Zb, unused;
		project<2>(r, s.x, s.y, 0.0f, Xa, unused, Za);
		project<2>(r, s.z, s.w, 0.0f, Xb, unused, Zb);
		hit = (Xa > 0.0f) != (Xb > 0.0f);
		if (!hit) { return false; }
		const double xa = Xa, xb = Xb, za = Za, zb = Zb;
		const double w = xa / (xa - xb);
		t = clamp_into(static_cast<float>(za + w * (zb - za)), fminf(Za, Zb), fmaxf(Za, Zb));
		if constexpr (BARY) { bary[0] = static_cast<float>(w); }
	}
	*t_out = t;
	return t >= t_min && t <= t_max;
}

// node k may hold a hit with t in [t_min, cut]; *zmin: the smallest Z of its box (an empty node: false)
template <int D>
__device__ inline bool node_admit(const Tree& tr, uint32_t k, const Ray& r, float t_min, float cut, float* zmin)
{
	const float4 lo = tr.box[2 * k], hi = tr.box[2 * k + 1];
	if (!(lo.x <= hi.x)) { return false; }
	const float lz = pick(lo, r.kz) - r.oz, hz = pick(hi, r.kz) - r.oz;
	const bool  xup = r.Sx >= 0.0f;
	const float xmin = (pick(lo, r.kx) - r.ox) - r.Sx * (xup ? hz : lz);
	const float xmax = (pick(hi, r.kx) - r.ox) - r.Sx * (xup ? lz : hz);
	bool prune = xmin > 0.0f || xmax < 0.0f;
	if constexpr (D == 3) {
		const bool  yup = r.Sy >= 0.0f;
		const float ymin = (pick(lo, r.ky) - r.oy) - r.Sy * (yup ? hz : lz);
		const float ymax = (pick(hi, r.ky) - r.oy) - r.Sy * (yup ? lz : hz);
		prune = prune || ymin > 0.0f || ymax < 0.0f;
	}
	const bool  zup = r.Sz > 0.0f;
	const float z0 = r.Sz * (zup ? lz : hz), z1 = r.Sz * (zup ? hz : lz);
	*zmin = z0;
	return !(prune || z1 < t_min || z0 > cut);
}

// bvh::search's walk with the ray's admission: cut() is the largest t that still matters, visit(i) judges sorted slot i
// and returns false to end the walk
template <int D, class Cut, class Visit>
__device__ inline void walk(const Tree& tr, const Ray& r, float t_min, Cut&& cut, Visit&& visit)
{
	if (tr.nf == 0) { return; }
	float z = 0.0f;
	if (!node_admit<D>(tr, 1, r, t_min, cut(), &z)) { return; }
	uint32_t k = 1, second = 0;
	int      depth = 0;
	for (;;) {
		if (depth == tr.H) {
			const int64_t b = static_cast<int64_t>(k - tr.P) * kRayLeaf;
			const int64_t e = b + kRayLeaf < tr.nf ? b + kRayLeaf : tr.nf;
			for (int64_t i = b; i < e; ++i) {
				if (!visit(i)) { return; }
			}
		} else {
			const float c  = cut();
			float       z0 = 0.0f, z1 = 0.0f;
			const bool  a0 = node_admit<D>(tr, 2 * k, r, t_min, c, &z0);
			const bool  a1 = node_admit<D>(tr, 2 * k + 1, r, t_min, c, &z1);
			if (a0 || a1) {
				k = 2 * k + ((a1 && (!a0 || z1 < z0)) ? 1u : 0u);  // the near child first (a tie: the left one)
				++depth;
				continue;
			}
		}
		for (;;) {
			if (depth == 0) { return; }
			const uint32_t bit = 1u << (depth - 1);
			if (!(second & bit)) {
				second |= bit;
				if (node_admit<D>(tr, k ^ 1u, r, t_min, cut(), &z)) {
					k ^= 1u;
					break;
				}
			}
			second &= ~bit;
			k >>= 1;
			--depth;
		}
	}
}

// what the counting kernel writes: counts (rays from buffers), containment (points, one direction), or the sign of the
// distances of points / of a lattice (+x)
enum { kCounts = 0, kInside = 1, kSign = 2, kSignLattice = 3 };

struct RayArgs {
	Tree           t;
	int64_t        n;
	const float*   o;       // float[n][D]: origins / points (not kSignLattice)
	const float*   d;       // float[n][D] (k_ray_hit, kCounts)
	float          dir[3];  // the one direction (kInside, kSign, kSignLattice)
	Lattice        l;       // kSignLattice
	float          t_min, t_max;
	int            limit;
	float*         hit_t;
	long long*     prim;    // or nullptr
	float*         bary;    // float[n][D - 1] or nullptr
	int*           counts;
	unsigned char* inside;
	float*         dist;    // kSign, kSignLattice: negated in place
};

template <int D>
__global__ __launch_bounds__(kThreads) void k_ray_hit(RayArgs a)
{
	const int64_t out = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (out >= a.n) { return; }
	float o[D], d[D];
#pragma unroll
	for (int e = 0; e < D; ++e) {
		o[e] = a.o[out * D + e];
		d[e] = a.d[out * D + e];
	}
	Ray        r;
	const bool ok   = ray_setup<D>(o, d, r);
	float      best = ok ? INFINITY : NAN;
	uint32_t   bidx = kNone;  // the smallest primitive index that reaches best, and its place in the sorted set
	int64_t    slot = -1;
	if (ok) {
		walk<D>(
		    a.t, r, a.t_min, [&]() { return fminf(best, a.t_max); },
		    [&](int64_t i) {
			    float    t = 0.0f;
			    uint32_t j = 0;
			    if (primitive_hit<D, false>(a.t, i, r, a.t_min, a.t_max, &t, &j, nullptr) && (t < best || (t == best && j < bidx))) {
				    best = t;
				    bidx = j;
				    slot = i;
			    }
			    return true;
		    });
	}
	a.hit_t[out] = best;
	if (a.prim) { a.prim[out] = index_of(bidx); }
	if (a.bary) {
		float b[2] = {NAN, NAN};
		if (bidx != kNone) {
			float    t = 0.0f;
			uint32_t j = 0;
			(void)primitive_hit<D, true>(a.t, slot, r, a.t_min, a.t_max, &t, &j, b);  // the same arithmetic: the same bits
		}
#pragma unroll
		for (int e = 0; e < D - 1; ++e) { a.bary[out * (D - 1) + e] = b[e]; }
	}
}

template <int D, int OUT>
__global__ __launch_bounds__(kThreads) void k_ray_count(RayArgs a)
{
	float   o[D], d[D];
	int64_t out;
	if constexpr (OUT == kSignLattice) {
		if (!lattice_query<D>(a.l, o, &out)) { return; }
	} else {
		out = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
		if (out >= a.n) { return; }
#pragma unroll
		for (int e = 0; e < D; ++e) { o[e] = a.o[out * D + e]; }
	}
#pragma unroll
	for (int e = 0; e < D; ++e) { d[e] = OUT == kCounts ? a.d[out * D + e] : a.dir[e]; }
	Ray      r;
	uint32_t count = 0;
	if (ray_setup<D>(o, d, r)) {
		const uint32_t limit = static_cast<uint32_t>(a.limit);
		walk<D>(
		    a.t, r, a.t_min, [&]() { return a.t_max; },
		    [&](int64_t i) {
			    float    t = 0.0f;
			    uint32_t j = 0;
			    count += primitive_hit<D, false>(a.t, i, r, a.t_min, a.t_max, &t, &j, nullptr) ? 1u : 0u;
			    return count < limit;  // saturated: nothing more to learn
		    });
	}
	if constexpr (OUT == kCounts) {
		a.counts[out] = static_cast<int>(count);
	} else if constexpr (OUT == kInside) {
		a.inside[out] = static_cast<unsigned char>(count & 1u);
	} else {
		if (count & 1u) { a.dist[out] = -a.dist[out]; }
	}
}

template <int OUT>
void launch_count(int D, dim3 grid, const RayArgs& a, hipStream_t st)
{
	if (D == 2) {
		hipLaunchKernelGGL((k_ray_count<2, OUT>), grid, dim3(kThreads), 0, st, a);
	} else {
		hipLaunchKernelGGL((k_ray_count<3, OUT>), grid, dim3(kThreads), 0, st, a);
	}
	FI_HIP_TRY(hipGetLastError());
}

// the rays of containment and of the sign: from each point along dir (null: +x), every hit from t = 0 on
void parity_rays(RayArgs& a, const SurfaceIndex& t, const float* direction)
{
	a.t      = tree_of(t);
	a.dir[0] = 1.0f;
	a.dir[1] = a.dir[2] = 0.0f;
	if (direction) {
		for (int d = 0; d < t.D; ++d) { a.dir[d] = direction[d]; }
	}
	a.t_min = 0.0f;
	a.t_max = INFINITY;
	a.limit = INT_MAX;
}

}  // namespace

void ray_cast(const SurfaceIndex& t, int64_t n, const float* origins, const float* directions, float t_min, float t_max, float* hit_t,
              long long* primitives, float* bary, int memory, hipStream_t st)
{
	if (n == 0) { return; }
	AllocStream alloc_on(st);
	Outputs     o(n, t.D - 1, hit_t, primitives, bary, memory);  // (its `closest`: D - 1 barycentrics per ray)
	stage::In<float> org(origins, n * t.D, memory, st), dir(directions, n * t.D, memory, st);
	RayArgs     a{};
	a.t     = tree_of(t);
	a.n     = n;
	a.o     = org;
	a.d     = dir;
	a.t_min = t_min;
	a.t_max = t_max;
	a.hit_t = o.dist;
	a.prim  = o.idx;
	a.bary  = o.cl;
	if (t.D == 2) {
		hipLaunchKernelGGL(k_ray_hit<2>, dim3(blocks_for(n)), dim3(kThreads), 0, st, a);
	} else {
		hipLaunchKernelGGL(k_ray_hit<3>, dim3(blocks_for(n)), dim3(kThreads), 0, st, a);
	}
	FI_HIP_TRY(hipGetLastError());
	o.finish(st);
}

void ray_count(const SurfaceIndex& t, int64_t n, const float* origins, const float* directions, float t_min, float t_max, int limit,
               int* counts, int memory, hipStream_t st)
{
	if (n == 0) { return; }
	AllocStream alloc_on(st);
	stage::In<float> org(origins, n * t.D, memory, st), dir(directions, n * t.D, memory, st);
	stage::Out<int>  c(counts, n, memory);
	RayArgs     a{};
	a.t      = tree_of(t);
	a.n      = n;
	a.o      = org;
	a.d      = dir;
	a.t_min  = t_min;
	a.t_max  = t_max;
	a.limit  = limit;
	a.counts = c;
	launch_count<kCounts>(t.D, dim3(blocks_for(n)), a, st);
	c.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

void ray_contains(const SurfaceIndex& t, int64_t n, const float* points, const float* direction, unsigned char* inside, int memory,
                  hipStream_t st)
{
	if (n == 0) { return; }
	AllocStream alloc_on(st);
	stage::In<float>           org(points, n * t.D, memory, st);
	stage::Out<unsigned char>  in(inside, n, memory);
	RayArgs     a{};
	parity_rays(a, t, direction);
	a.n      = n;
	a.o      = org;
	a.inside = in;
	launch_count<kInside>(t.D, dim3(blocks_for(n)), a, st);
	in.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

void ray_signed_query(const SurfaceIndex& t, int64_t n, const float* queries, float max_distance, float* distances,
                      long long* primitives, float* closest, int memory, hipStream_t st)
{
	if (n == 0) { return; }
	AllocStream alloc_on(st);
	Outputs     o(n, t.D, distances, primitives, closest, memory);
	stage::In<float> q(queries, n * t.D, memory, st);
	RayArgs     a{};
	parity_rays(a, t, nullptr);
	a.n    = n;
	a.o    = q;
	a.dist = o.dist;
	surface_query(t, n, a.o, max_distance, o.dist, o.idx, o.cl, FI_DEVICE, st);  // the unchanged kernels, on the device
	launch_count<kSign>(t.D, dim3(blocks_for(n)), a, st);
	o.finish(st);
}

void ray_signed_lattice(const SurfaceIndex& t, const int* sizes, float max_distance, float* out, long long* primitives, int memory,
                        hipStream_t st)
{
	RayArgs     a{};
	int64_t     total = 0;
	const dim3  grid  = lattice_grid(t.D, sizes, a.l, &total);
	AllocStream alloc_on(st);
	Outputs     o(total, t.D, out, primitives, nullptr, memory);
	parity_rays(a, t, nullptr);
	a.n    = total;
	a.dist = o.dist;
	surface_lattice(t, sizes, max_distance, o.dist, o.idx, FI_DEVICE, st);
	launch_count<kSignLattice>(t.D, grid, a, st);
	o.finish(st);
}

}  // namespace fi
