// fi_march.hip -- rays and pinhole images of a lattice field or a depth volume, on the device.  A ray is clipped to the
// lattice's box, sampled every `step` lattice units through the trilinear (2-D: bilinear) interpolant, and the first pair of
// valid samples that the iso-level separates is refined by a fixed number of bisections and one linear interpolation; the
// hit's normal is the interpolant's unit gradient.  The contract is include/fi_hip.h (fi_field_raycast, fi_field_render),
// tests/march_reference.py its definition in numpy; DESIGN.md 4.28.  All arithmetic is fp32, one rounding per operation (the
// tree's -ffp-contract=off); a ray is its thread's own, nothing is accumulated across threads, so every output is defined bit
// for bit.  One __device__ core (march) serves both kernels: k_march_rays, a thread per ray in input order, and
// k_march_image, where a wave owns an 8 x 8 pixel tile so that its 64 rays stay within a few cells of one another and
// their corner gathers fall into the same cache lines.  The march is a gather loop bound by latency: a thread keeps the 2^D
// corners of its current cell in registers (four 8-byte loads in 3-D, four more for the weights, which collapse into one
// flag) and reloads only when the sample's cell changes.  No LDS, no scratch, no atomics.
#include "fi_march.h"

#include <cmath>
#include <cstring>

#include "fi_depth.h"
#include "fi_stage.h"

namespace fi {
namespace {

constexpr int kMarchThreads = 256;
constexpr int kTile         = 8;  // a wave's pixels: kTile x kTile
static_assert(kTile * kTile == 64, "a wave owns one tile, a lane one pixel");

struct MarchArgs {  // wave-uniform: kernel arguments, scalar registers
	const float* f;
	const float* w;
	int          n[3];
	float        iso, step, min_weight;
	int          refine, side;
};

struct CamArgs {  // the camera of an image as k_march_image reads it, and the tiling
	float    r[12];  // rows of [R | t]
	float    fx, fy, cx, cy;
	int      width, height, kind;
	unsigned tiles_x, ntiles;
};

// two x-adjacent samples in one 8-byte load (the address is a multiple of 4 only)
struct __attribute__((packed, aligned(4))) Pair {
	float a, b;
};

__device__ __forceinline__ bool finite_(float v) { return fabsf(v) < INFINITY; }

// A ray's march state: the ray, the box, and the cell whose corners are in registers.
template <int D, bool W>
struct Marcher {
	const MarchArgs& a;
	float            o[D], d[D], hi[D];
	int              at = -1;  // linear index of the cached cell's corner 0
	float            fv[1 << D];
	bool             ok = false;  // the cached cell's weights admit it

	__device__ __forceinline__ Marcher(const MarchArgs& args) : a(args) {}

	__device__ __forceinline__ void load(int idx)
	{
		at = idx;
		const int sy = a.n[0], sz = a.n[0] * a.n[1];
#pragma unroll
		for (int k = 0; k < (1 << (D - 1)); ++k) {
			const int  q = idx + ((k & 1) ? sy : 0) + ((k & 2) ? sz : 0);
			const Pair p = *reinterpret_cast<const Pair*>(a.f + q);
			fv[2 * k]     = p.a;
			fv[2 * k + 1] = p.b;
		}
		ok = true;
		if (W) {
#pragma unroll
			for (int k = 0; k < (1 << (D - 1)); ++k) {
				const int  q = idx + ((k & 1) ? sy : 0) + ((k & 2) ? sz : 0);
				const Pair p = *reinterpret_cast<const Pair*>(a.w + q);
				ok = ok && p.a > 0.0f && p.a >= a.min_weight && p.b > 0.0f && p.b >= a.min_weight;
			}
		}
	}

	// the sample at t: its position p, its offsets' weights u, its value; valid: the cell is admitted and the value finite
	__device__ __forceinline__ float eval(float t, float (&p)[D], float (&u)[D][2], bool& valid)
	{
		int c[D];
#pragma unroll
		for (int j = 0; j < D; ++j) {
			float q = o[j] + t * d[j];
			q       = q > 0.0f ? (q > hi[j] ? hi[j] : q) : 0.0f;  // (NaN: 0; always inside the box)
			p[j]    = q;
			c[j]    = min(static_cast<int>(floorf(q)), a.n[j] - 2);
			const float s = q - static_cast<float>(c[j]);
			u[j][0] = 1.0f - s;
			u[j][1] = s;
		}
		int idx = c[0] + a.n[0] * c[1];
		if (D == 3) { idx += a.n[0] * a.n[1] * c[2]; }
		if (idx != at) { load(idx); }
		float v = 0.0f;
#pragma unroll
		for (int k = 0; k < (1 << D); ++k) {
			float w = u[0][k & 1];
#pragma unroll
			for (int j = 1; j < D; ++j) { w = w * u[j][(k >> j) & 1]; }
			const float term = w * fv[k];
			v = k == 0 ? term : v + term;
		}
		valid = ok && finite_(v);
		return v;
	}

	// the unit gradient of the cached cell at the offsets u: zero unless its length is > 0 and finite
	__device__ __forceinline__ void normal(const float (&u)[D][2], float (&n)[D]) const
	{
		float g[D];
#pragma unroll
		for (int j = 0; j < D; ++j) {
			float acc   = 0.0f;
			bool  first = true;
#pragma unroll
			for (int k = 0; k < (1 << D); ++k) {
				if ((k >> j) & 1) { continue; }
				float w    = 1.0f;
				bool  have = false;
#pragma unroll
				for (int e = 0; e < D; ++e) {
					if (e == j) { continue; }
					w    = have ? w * u[e][(k >> e) & 1] : u[e][(k >> e) & 1];
					have = true;
				}
				const float term = w * (fv[k | (1 << j)] - fv[k]);
				acc   = first ? term : acc + term;
				first = false;
			}
			g[j] = acc;
		}
		float l2 = g[0] * g[0] + g[1] * g[1];
		if (D == 3) { l2 = l2 + g[2] * g[2]; }
		const float len  = sqrtf(l2);
		const bool  good = len > 0.0f && len < INFINITY;
#pragma unroll
		for (int j = 0; j < D; ++j) { n[j] = good ? g[j] / len : 0.0f; }
	}
};

template <int D>
__device__ __forceinline__ float length(const float (&d)[D])
{
	float l2 = d[0] * d[0] + d[1] * d[1];
	if (D == 3) { l2 = l2 + d[2] * d[2]; }
	return sqrtf(l2);
}

// The march of one ray (include/fi_hip.h, steps 1 to 6) -> t, the hit's position and normal, side (+1, -1, or 0: no hit).
template <int D, bool W>
__device__ __forceinline__ void march(const MarchArgs& a, const float (&o)[D], const float (&d)[D], float t_min, float t_max, float& t,
                                      float (&pos)[D], float (&nrm)[D], int& side)
{
	Marcher<D, W> m(a);
	bool          fin = true;
#pragma unroll
	for (int j = 0; j < D; ++j) {
		m.o[j]  = o[j];
		m.d[j]  = d[j];
		m.hi[j] = static_cast<float>(a.n[j] - 1);
		pos[j]  = NAN;
		nrm[j]  = 0.0f;
		fin     = fin && finite_(o[j]) && finite_(d[j]);
	}
	side = 0;
	t    = NAN;
	const float len = length<D>(d);
	if (!fin || !(len > 0.0f && len < INFINITY)) { return; }  // no ray
	t = INFINITY;
	float te = -INFINITY, tx = INFINITY;
	bool  miss = false;
#pragma unroll
	for (int j = 0; j < D; ++j) {
		if (d[j] == 0.0f) {
			miss = miss || !(o[j] >= 0.0f && o[j] <= m.hi[j]);
		} else {
			const float u = (0.0f - o[j]) / d[j], v = (m.hi[j] - o[j]) / d[j];
			const float lo = u < v ? u : v, up = u > v ? u : v;
			te = te > lo ? te : lo;
			tx = tx < up ? tx : up;
		}
	}
	const float ta = te > t_min ? te : t_min, tb = tx < t_max ? tx : t_max;
	if (miss || ta > tb || !finite_(ta) || !finite_(tb)) { return; }
	const float dt = a.step / len;
	if (!(dt > 0.0f && dt < INFINITY)) { return; }

	float p[D], u[D][2];
	float pt = 0.0f, pf = 0.0f;  // the previous sample
	bool  pv = false;
	float ha = 0.0f, hb = 0.0f, fa = 0.0f, fb = 0.0f;  // the bracket
	int   hs = 0;
	for (int k = 0; k < FI_MARCH_MAX_SAMPLES; ++k) {
		const float raw = ta + static_cast<float>(k) * dt;
		const float tk  = raw < tb ? raw : tb;
		bool        v;
		const float f = m.eval(tk, p, u, v);
		if (pv && v) {
			const bool ip = pf < a.iso, ic = f < a.iso;
			if (!ip && ic && a.side != FI_MARCH_BACK) {
				hs = 1;
			} else if (ip && !ic && a.side != FI_MARCH_FRONT) {
				hs = -1;
			}
			if (hs != 0) {
				ha = pt;
				hb = tk;
				fa = pf;
				fb = f;
				break;
			}
		}
		pt = tk;
		pf = f;
		pv = v;
		if (!(raw < tb)) { break; }
	}
	if (hs == 0) { return; }
	for (int r = 0; r < a.refine; ++r) {
		const float mid = 0.5f * (ha + hb);
		bool        v;
		const float f = m.eval(mid, p, u, v);
		if (!v) { break; }
		if ((f < a.iso) == (fa < a.iso)) {
			ha = mid;
			fa = f;
		} else {
			hb = mid;
			fb = f;
		}
	}
	t = ha + ((fa - a.iso) / (fa - fb)) * (hb - ha);
	bool v;
	m.eval(t, pos, u, v);
	m.normal(u, nrm);
	side = hs;
}

template <int D, bool W>
__global__ __launch_bounds__(kMarchThreads) void k_march_rays(MarchArgs a, int64_t n, const float* __restrict__ origins,
                                                               const float* __restrict__ directions, float t_min, float t_max,
                                                               float* __restrict__ t, float* __restrict__ positions,
                                                               float* __restrict__ normals, signed char* __restrict__ side)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kMarchThreads + threadIdx.x;
	if (i >= n) { return; }
	float o[D], d[D], pos[D], nrm[D], th;
	int   s;
#pragma unroll
	for (int j = 0; j < D; ++j) {
		o[j] = origins[i * D + j];
		d[j] = directions[i * D + j];
	}
	march<D, W>(a, o, d, t_min, t_max, th, pos, nrm, s);
	if (t) { t[i] = th; }
	if (side) { side[i] = static_cast<signed char>(s); }
#pragma unroll
	for (int j = 0; j < D; ++j) {
		if (positions) { positions[i * D + j] = pos[j]; }
		if (normals) { normals[i * D + j] = nrm[j]; }
	}
}

// A wave owns tile (ty, tx) of kTile x kTile pixels, lane l pixel (ty kTile + l / kTile, tx kTile + l % kTile): every pixel
// of the image belongs to exactly one lane of one wave, and the lanes beyond the image's edge leave at once.
template <bool W>
__global__ __launch_bounds__(kMarchThreads) void k_march_image(MarchArgs a, CamArgs c, float* __restrict__ depth,
                                                                float* __restrict__ positions, float* __restrict__ normals,
                                                                float* __restrict__ incidence)
{
	const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int      lane = threadIdx.x & 63;
	const unsigned tile = blockIdx.x * (kMarchThreads / 64) + wave;
	if (tile >= c.ntiles) { return; }
	const int row = static_cast<int>(tile / c.tiles_x) * kTile + lane / kTile;
	const int col = static_cast<int>(tile % c.tiles_x) * kTile + lane % kTile;
	if (row >= c.height || col >= c.width) { return; }
	const float px = ((static_cast<float>(col) + 0.5f) - c.cx) / c.fx;
	const float py = ((static_cast<float>(row) + 0.5f) - c.cy) / c.fy;
	const float e0 = 0.0f - c.r[3], e1 = 0.0f - c.r[7], e2 = 0.0f - c.r[11];
	float       o[3], d[3], pos[3], nrm[3], t;
	int         s;
#pragma unroll
	for (int j = 0; j < 3; ++j) {
		o[j] = (c.r[j] * e0 + c.r[4 + j] * e1) + c.r[8 + j] * e2;
		d[j] = (c.r[j] * px + c.r[4 + j] * py) + c.r[8 + j];
	}
	march<3, W>(a, o, d, 0.0f, INFINITY, t, pos, nrm, s);
	const bool hit = s != 0;
	float      q   = 0.0f;
	if (hit) {
		const float len = length<3>(d);
		const float dot = (nrm[0] * (d[0] / len) + nrm[1] * (d[1] / len)) + nrm[2] * (d[2] / len);
		q = -dot;
		q = q < 1.0f ? q : 1.0f;
	}
	if (!(q > 0.0f)) {  // no hit, a back hit or no normal
		q = 0.0f;
		nrm[0] = nrm[1] = nrm[2] = 0.0f;
	}
	const int64_t i = static_cast<int64_t>(row) * c.width + col;
	float         z = INFINITY;
	if (hit) { z = c.kind == FI_DEPTH_Z ? t : t * sqrtf((px * px + py * py) + 1.0f); }
	depth[i] = z;
#pragma unroll
	for (int j = 0; j < 3; ++j) {
		if (positions) { positions[3 * i + j] = pos[j]; }
		if (normals) { normals[3 * i + j] = nrm[j]; }
	}
	if (incidence) { incidence[i] = q; }
}

MarchArgs args_of(const MarchField& field, const fi_march_options& o)
{
	MarchArgs a{};
	a.f = field.f;
	a.w = field.w;
	for (int j = 0; j < 3; ++j) { a.n[j] = j < field.ndim ? field.n[j] : 1; }
	a.iso        = o.iso;
	a.step       = o.step;
	a.min_weight = o.min_weight;
	a.refine     = o.refine;
	a.side       = o.side;
	return a;
}

}  // namespace

int64_t check_march_field(int ndim, const int* sizes)
{
	FI_REQUIRE(sizes != nullptr, FI_ERR_INVALID, "sizes is null");
	FI_REQUIRE(ndim >= 1 && ndim <= 3, FI_ERR_INVALID, "ndim must be 1, 2 or 3 (got %d)", ndim);
	FI_REQUIRE(ndim >= 2, FI_ERR_UNSUPPORTED, "rays against a 1-D field are not supported");
	int64_t total = 1;
	for (int j = 0; j < ndim; ++j) {
		FI_REQUIRE(sizes[j] >= 2, FI_ERR_INVALID, "marching needs sizes >= 2 (sizes[%d] = %d)", j, sizes[j]);
		total *= sizes[j];
		// (a thread keeps a cell's linear index in 32 bits)
		FI_REQUIRE(total < (int64_t(1) << 31), FI_ERR_UNSUPPORTED, "a lattice of 2^31 points or more");
	}
	return total;
}

void check_march_options(const fi_march_options* o)
{
	FI_REQUIRE(o != nullptr, FI_ERR_INVALID, "options is null");
	FI_REQUIRE(std::isfinite(o->iso), FI_ERR_INVALID, "iso is not finite");
	FI_REQUIRE(o->step > 0.0f && std::isfinite(o->step), FI_ERR_INVALID, "step must be > 0 and finite (got %g)", static_cast<double>(o->step));
	FI_REQUIRE(o->refine >= 0 && o->refine <= 16, FI_ERR_INVALID, "refine must be 0 .. 16 (got %d)", o->refine);
	FI_REQUIRE(o->side == FI_MARCH_FRONT || o->side == FI_MARCH_BACK || o->side == FI_MARCH_EITHER, FI_ERR_INVALID, "bad side %d", o->side);
	FI_REQUIRE(o->min_weight == o->min_weight, FI_ERR_INVALID, "min_weight is NaN");
}

void march_rays(const MarchField& field, const fi_march_options& o, int64_t n, const float* origins, const float* directions,
                float t_min, float t_max, float* t, float* positions, float* normals, signed char* side, int memory, hipStream_t st)
{
	if (n == 0) { return; }
	const int                D = field.ndim;
	AllocStream              alloc_on(st);
	stage::In<float>         og(origins, D * n, memory, st), dr(directions, D * n, memory, st);
	stage::Out<float>        th(t, n, memory), po(positions, D * n, memory), nr(normals, D * n, memory);
	stage::Out<signed char>  sd(side, n, memory);
	const MarchArgs          a = args_of(field, o);
	const dim3               grid(static_cast<unsigned>((n + kMarchThreads - 1) / kMarchThreads)), block(kMarchThreads);
	auto launch = [&](auto kernel) {
		hipLaunchKernelGGL(kernel, grid, block, 0, st, a, n, og.dev, dr.dev, t_min, t_max, th.dev, po.dev, nr.dev, sd.dev);
	};
	if (D == 2) {
		field.w ? launch(k_march_rays<2, true>) : launch(k_march_rays<2, false>);
	} else {
		field.w ? launch(k_march_rays<3, true>) : launch(k_march_rays<3, false>);
	}
	FI_HIP_TRY(hipGetLastError());
	th.back(st);
	po.back(st);
	nr.back(st);
	sd.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

void march_image(const MarchField& field, const fi_march_options& o, const fi_camera& cam, float* depth, float* positions,
                 float* normals, float* incidence, int memory, hipStream_t st)
{
	const int64_t n = camera_pixels(cam);
	CamArgs       c{};
	std::memcpy(c.r, cam.pose, sizeof(c.r));
	c.fx     = cam.fx;
	c.fy     = cam.fy;
	c.cx     = cam.cx;
	c.cy     = cam.cy;
	c.width  = cam.width;
	c.height = cam.height;
	c.kind   = cam.kind;
	const int64_t tiles_x = (cam.width + kTile - 1) / kTile, tiles_y = (cam.height + kTile - 1) / kTile;
	FI_REQUIRE(tiles_x * tiles_y < (int64_t(1) << 31), FI_ERR_UNSUPPORTED, "%lld tiles in one image", static_cast<long long>(tiles_x * tiles_y));
	c.tiles_x = static_cast<unsigned>(tiles_x);
	c.ntiles  = static_cast<unsigned>(tiles_x * tiles_y);
	AllocStream       alloc_on(st);
	stage::Out<float> de(depth, n, memory), po(positions, 3 * n, memory), nr(normals, 3 * n, memory), in(incidence, n, memory);
	const MarchArgs   a = args_of(field, o);
	const int         per = kMarchThreads / 64;
	const dim3        grid((c.ntiles + per - 1) / per), block(kMarchThreads);
	if (field.w) {
		hipLaunchKernelGGL(k_march_image<true>, grid, block, 0, st, a, c, de.dev, po.dev, nr.dev, in.dev);
	} else {
		hipLaunchKernelGGL(k_march_image<false>, grid, block, 0, st, a, c, de.dev, po.dev, nr.dev, in.dev);
	}
	FI_HIP_TRY(hipGetLastError());
	de.back(st);
	po.back(st);
	nr.back(st);
	in.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

}  // namespace fi
