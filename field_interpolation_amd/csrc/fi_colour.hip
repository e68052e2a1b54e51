// fi_colour.hip -- colour in a depth volume.  A volume may carry up to four planar fp32 channels and one colour weight per
// voxel.  The fusion is the depth unit's voxel-stationary pass with more state: a thread owns a voxel, runs steps 1 - 8 of
// fi_volume_integrate through the body both units share (fi_volume_pass.h) and, where the voxel lies in the colour band,
// averages the pixel's colour into its channels.  The colour at a point is the average of the observed corners of its cell
// under the trilinear weights; an image's colours are that at every hit of fi_volume_render; the coloured voxels leave as data
// points by the mark / scan / gather of fi_volume_constraints.  The contract is include/fi_hip.h (fi_volume_integrate_colour,
// fi_volume_colour_sample), tests/colour_reference.py its definition in numpy; DESIGN.md 4.29.  All arithmetic is fp32, one
// rounding per operation (the tree's -ffp-contract=off); no atomics, no LDS.
#include "fi_colour.h"

#include <cmath>
#include <cstdint>

#include "fi_march.h"
#include "fi_prim.h"
#include "fi_solver_internal.h"
#include "fi_stage.h"
#include "fi_volume_pass.h"

namespace fi {
namespace {

static_assert(kThreads == prim::kGridThreads, "grid() counts work groups of kThreads");

// ---- fusion -----------------------------------------------------------------------------------------------------------------
// the C channels of pixel `pix`: C consecutive floats, one 8- or 16-byte load where Vec says the images' address allows it
template <int C, bool Vec>
__device__ __forceinline__ void pixel_of(const float* __restrict__ colours, int64_t pix, float (&c)[C])
{
	const float* p = colours + C * pix;
	if constexpr (Vec && C == 4) {
		const float4 v = *reinterpret_cast<const float4*>(p);
		c[0] = v.x, c[1] = v.y, c[2] = v.z, c[3] = v.w;
	} else if constexpr (Vec && C == 2) {
		const float2 v = *reinterpret_cast<const float2*>(p);
		c[0] = v.x, c[1] = v.y;
	} else {
#pragma unroll
		for (int k = 0; k < C; ++k) { c[k] = p[k]; }
	}
}

// k_volume_integrate with the colour state beside tsdf and W: the voxel's Wc and C channels are read once, up to kCams images
// are applied in image order and every array is written once.  Steps 9 - 11 of fi_volume_integrate_colour follow step 8 of an
// image; a colour skip leaves the geometry update as it is.  The loop counter is wave-uniform: the cameras stay in scalar
// registers.  The pixel's colour is one gather of C consecutive floats.  No LDS, no atomics.
template <int C, bool Vec>
__global__ __launch_bounds__(kThreads) void k_colour_integrate(VolArgs a, const CamTable* __restrict__ tab, int nc,
                                                                const float* __restrict__ depth, const float* __restrict__ inc,
                                                                const float* __restrict__ iw, float min_inc,
                                                                const float* __restrict__ colours, float band, int64_t nvox,
                                                                float* __restrict__ tsdf, float* __restrict__ weight,
                                                                float* __restrict__ chan, float* __restrict__ cweight)
{
	const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int      lane = threadIdx.x & 63;
	const unsigned wid  = blockIdx.x * (kThreads / 64) + wave;
	if (wid >= a.nwaves) { return; }
	const WaveRun            r = run_of(a, wid);
	const unsigned long long culled = culled_of(tab, nc, r, lane);

	const int x = r.x0 + lane;
	if (x > r.x1) { return; }
	const int64_t idx = (static_cast<int64_t>(r.z) * a.ny + r.y) * a.nx + x;
	const float   X = static_cast<float>(x), Y = static_cast<float>(r.y), Z = static_cast<float>(r.z);
	float         t = tsdf[idx], W = weight[idx], Wc = cweight[idx];
	float         A[C];
#pragma unroll
	for (int k = 0; k < C; ++k) { A[k] = chan[k * nvox + idx]; }
	for (int s = 0; s < nc; ++s) {
		if (image_culled(culled, s)) { continue; }
		VoxelSample v;
		if (!voxel_sample(a, tab->cam[s], X, Y, Z, depth, inc, iw, min_inc, v)) { continue; }
		voxel_fuse(a, v, t, W);
		if (!(fabsf(v.g) < band)) { continue; }
		float c[C];
		pixel_of<C, Vec>(colours, v.pix, c);
		bool finite = true;
#pragma unroll
		for (int k = 0; k < C; ++k) { finite = finite && fabsf(c[k]) < INFINITY; }
		if (!finite) { continue; }
		const float sum = Wc + v.w;
#pragma unroll
		for (int k = 0; k < C; ++k) { A[k] = (A[k] * Wc + c[k] * v.w) / sum; }
		Wc = sum < a.max_weight ? sum : a.max_weight;
	}
	tsdf[idx]    = t;
	weight[idx]  = W;
	cweight[idx] = Wc;
#pragma unroll
	for (int k = 0; k < C; ++k) { chan[k * nvox + idx] = A[k]; }
}

// ---- the colour at a point --------------------------------------------------------------------------------------------------
struct SampleArgs {
	int     nx, ny, nz;
	int64_t nvox;
	float   min_weight;
};

// one axis of the cell of p: the lower corner (as an index and as a float) and the two weights; p is inside [0, hi]
__device__ __forceinline__ void axis_of(float p, int size, int& cell, float& w0, float& w1)
{
	const float fl = floorf(p), top = static_cast<float>(size - 2);
	const float cf = fl < top ? fl : top;
	const float t  = p - cf;
	cell = static_cast<int>(cf);
	w0   = 1.0f - t;
	w1   = t;
}

// A thread per point: the corners of its cell in ascending a + 2 b + 4 c, those with an observed colour (Wc > 0 and Wc >=
// min_weight) summed under omega = (wx_a wy_b) wz_c, the colour normalised over what was summed.
template <int C>
__global__ __launch_bounds__(kThreads) void k_colour_sample(SampleArgs a, int64_t n, const float* __restrict__ positions,
                                                             const float* __restrict__ chan, const float* __restrict__ cweight,
                                                             float* __restrict__ colours, unsigned char* __restrict__ valid)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	const float px = positions[3 * i + 0], py = positions[3 * i + 1], pz = positions[3 * i + 2];
	const float hx = static_cast<float>(a.nx - 1), hy = static_cast<float>(a.ny - 1), hz = static_cast<float>(a.nz - 1);
	float       S = 0.0f, N[C];
#pragma unroll
	for (int k = 0; k < C; ++k) { N[k] = 0.0f; }
	// (a NaN fails every compare, an infinity one of them)
	if (px >= 0.0f && px <= hx && py >= 0.0f && py <= hy && pz >= 0.0f && pz <= hz) {
		int   cx, cy, cz;
		float wx[2], wy[2], wz[2];
		axis_of(px, a.nx, cx, wx[0], wx[1]);
		axis_of(py, a.ny, cy, wy[0], wy[1]);
		axis_of(pz, a.nz, cz, wz[0], wz[1]);
		const int64_t base = (static_cast<int64_t>(cz) * a.ny + cy) * a.nx + cx;
#pragma unroll
		for (int corner = 0; corner < 8; ++corner) {
			const int     ia = corner & 1, ib = (corner >> 1) & 1, ic = corner >> 2;
			const float   omega = (wx[ia] * wy[ib]) * wz[ic];
			const int64_t idx = base + (static_cast<int64_t>(ic) * a.ny + ib) * a.nx + ia;
			const float   Wc = cweight[idx];
			if (Wc > 0.0f && Wc >= a.min_weight) {
				S = S + omega;
#pragma unroll
				for (int k = 0; k < C; ++k) { N[k] = N[k] + omega * chan[k * a.nvox + idx]; }
			}
		}
	}
	const bool ok = S > 0.0f;
#pragma unroll
	for (int k = 0; k < C; ++k) { colours[C * i + k] = ok ? N[k] / S : NAN; }
	if (valid) { valid[i] = ok ? 1 : 0; }
}

// ---- the coloured voxels as data points -------------------------------------------------------------------------------------
// flag[i] = 1 for a voxel with an observed colour, flag[n] = 0: the exclusive sums' last entry is the count
__global__ __launch_bounds__(kThreads) void k_colour_mark(int64_t n, const float* __restrict__ cweight, float min_weight,
                                                           uint32_t* __restrict__ flag)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i > n) { return; }
	uint32_t f = 0;
	if (i < n) {
		const float Wc = cweight[i];
		f = (Wc > 0.0f && Wc >= min_weight) ? 1u : 0u;
	}
	flag[i] = f;
}

__global__ __launch_bounds__(kThreads) void k_colour_gather(int nx, int ny, int channels, float max_weight, int64_t n, int64_t capacity,
                                                             const float* __restrict__ chan, const float* __restrict__ cweight,
                                                             const uint32_t* __restrict__ flag, const uint32_t* __restrict__ slot,
                                                             float* __restrict__ positions, float* __restrict__ colours,
                                                             float* __restrict__ weights)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n || !flag[i]) { return; }
	const int64_t o = slot[i];
	if (o >= capacity) { return; }
	if (positions) {
		const int64_t plane = static_cast<int64_t>(nx) * ny;
		const int64_t in_plane = i % plane;
		positions[3 * o + 0] = static_cast<float>(in_plane % nx);
		positions[3 * o + 1] = static_cast<float>(in_plane / nx);
		positions[3 * o + 2] = static_cast<float>(i / plane);
	}
	if (colours) {
		for (int k = 0; k < channels; ++k) { colours[channels * o + k] = chan[k * n + i]; }
	}
	if (weights) { weights[o] = cweight[i] / max_weight; }
}

template <int C>
void launch_sample(const fi_volume* v, float min_weight, int64_t n, const float* positions, float* colours, unsigned char* valid,
                   hipStream_t st)
{
	const SampleArgs a{v->n[0], v->n[1], v->n[2], v->nvox, min_weight};
	hipLaunchKernelGGL(k_colour_sample<C>, prim::grid(n), dim3(kThreads), 0, st, a, n, positions, v->colour.as<float>(),
	                   v->colour_weight.as<float>(), colours, valid);
}

// positions, colours and valid are on the device
void sample_on_device(const fi_volume* v, float min_weight, int64_t n, const float* positions, float* colours, unsigned char* valid,
                      hipStream_t st)
{
	switch (v->channels) {
	case 1: launch_sample<1>(v, min_weight, n, positions, colours, valid, st); break;
	case 2: launch_sample<2>(v, min_weight, n, positions, colours, valid, st); break;
	case 3: launch_sample<3>(v, min_weight, n, positions, colours, valid, st); break;
	default: launch_sample<4>(v, min_weight, n, positions, colours, valid, st); break;
	}
	FI_HIP_TRY(hipGetLastError());
}

bool aligned(const void* p, uintptr_t bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; }

}  // namespace

void volume_set_channels(fi_volume* v, int channels, hipStream_t st)
{
	AllocStream alloc_on(st);
	v->colour.alloc(sizeof(float) * channels * v->nvox);
	v->colour_weight.alloc(sizeof(float) * v->nvox);
	FI_HIP_TRY(hipMemsetAsync(v->colour.p, 0, sizeof(float) * channels * v->nvox, st));  // (all bits zero: 0.0f)
	FI_HIP_TRY(hipMemsetAsync(v->colour_weight.p, 0, sizeof(float) * v->nvox, st));
	FI_HIP_TRY(hipStreamSynchronize(st));
	v->channels = channels;
}

void volume_integrate_colour(fi_volume* v, long m, const fi_camera* cameras, const float* depths, const float* incidences,
                             const float* image_weights, float min_incidence, const float* colours, float band, int memory,
                             hipStream_t st)
{
	if (m == 0) { return; }
	const int                   C = v->channels;
	const VolArgs               a = args_of(v);
	int64_t                     pixels = 0;
	const std::vector<CamTable> host = tables_of(v, m, cameras, &pixels);
	const long                  launches = static_cast<long>(host.size());
	AllocStream                 alloc_on(st);
	const float *               d = nullptr, *q = nullptr, *iw = nullptr, *col = nullptr;
	const CamTable*             tab = nullptr;
	DevBuf                      block;
	prim::arena_alloc(block, [&](prim::Arena& ar) {
		tab = stage::in(ar, host.data(), launches, FI_HOST, st);
		d   = stage::in(ar, depths, pixels, memory, st);
		q   = stage::in(ar, incidences, pixels, memory, st);
		iw  = stage::in(ar, image_weights, m, memory, st);
		col = stage::in(ar, colours, C * pixels, memory, st);
	});
	const dim3 grid((a.nwaves + kThreads / 64 - 1) / (kThreads / 64));
	for (long l = 0; l < launches; ++l) {
		const int nc = static_cast<int>(std::min<long>(kCams, m - l * kCams));
		auto      launch = [&](auto kernel) {
			hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, st, a, tab + l, nc, d, q, iw, min_incidence, col, band, v->nvox,
			                   v->tsdf.as<float>(), v->weight.as<float>(), v->colour.as<float>(), v->colour_weight.as<float>());
		};
		// (a pixel's channels start at a multiple of C floats past `col`: aligned wherever `col` is)
		switch (C) {
		case 1: launch(k_colour_integrate<1, false>); break;
		case 2: aligned(col, 8) ? launch(k_colour_integrate<2, true>) : launch(k_colour_integrate<2, false>); break;
		case 3: launch(k_colour_integrate<3, false>); break;
		default: aligned(col, 16) ? launch(k_colour_integrate<4, true>) : launch(k_colour_integrate<4, false>); break;
		}
		FI_HIP_TRY(hipGetLastError());
	}
	FI_HIP_TRY(hipStreamSynchronize(st));  // (the table and the staged images live until here)
}

void volume_colour_sample(const fi_volume* v, float min_weight, int64_t n, const float* positions, float* colours, unsigned char* valid,
                          int memory, hipStream_t st)
{
	if (n == 0) { return; }
	AllocStream               alloc_on(st);
	stage::In<float>          po(positions, 3 * n, memory, st);
	stage::Out<float>         co(colours, v->channels * n, memory);
	stage::Out<unsigned char> va(valid, n, memory);
	sample_on_device(v, min_weight, n, po.dev, co.dev, va.dev, st);
	co.back(st);
	va.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

void volume_render_colour(const fi_volume* v, const fi_march_options& o, const fi_camera& cam, float colour_min_weight, float* depth,
                          float* positions, float* normals, float* incidence, float* colours, int memory, hipStream_t st)
{
	const int64_t     n = camera_pixels(cam);
	AllocStream       alloc_on(st);
	stage::Out<float> de(depth, n, memory), po(positions, 3 * n, memory), nr(normals, 3 * n, memory), in(incidence, n, memory);
	stage::Out<float> co(colours, v->channels * n, memory);
	DevBuf            own;  // the hit positions where the caller wants none
	float*            hits = po.dev;
	if (!hits) {
		own.alloc(sizeof(float) * 3 * n);
		hits = own.as<float>();
	}
	// the render fi_volume_render runs, on device buffers; a pixel without a hit has a NaN position and so a NaN colour
	const MarchField field{v->tsdf.as<float>(), v->weight.as<float>(), 3, {v->n[0], v->n[1], v->n[2]}};
	march_image(field, o, cam, de.dev, hits, nr.dev, in.dev, FI_DEVICE, st);
	sample_on_device(v, colour_min_weight, n, hits, co.dev, nullptr, st);
	de.back(st);
	po.back(st);
	nr.back(st);
	in.back(st);
	co.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

int64_t volume_colour_constraints(const fi_volume* v, float min_weight, int64_t capacity, float* positions, float* colours, float* weights,
                                  int memory, hipStream_t st)
{
	AllocStream   alloc_on(st);
	DevBuf        block;
	uint32_t *    flag = nullptr, *slot = nullptr;
	const int64_t n = v->nvox;
	prim::Scratch tmp;
	prim::arena_alloc(block, [&](prim::Arena& ar) {
		flag      = ar.take<uint32_t>(n + 1);
		slot      = ar.take<uint32_t>(n + 1);
		tmp.bytes = prim::scan_bytes(n + 1);
		tmp.p     = ar.take<char>(static_cast<int64_t>(tmp.bytes));
	});
	hipLaunchKernelGGL(k_colour_mark, prim::grid(n + 1), dim3(kThreads), 0, st, n, v->colour_weight.as<float>(), min_weight, flag);
	FI_HIP_TRY(hipGetLastError());
	prim::scan_u32(flag, slot, n + 1, tmp, st);
	const int64_t count = prim::read_u32(slot + n, st);
	if ((!positions && !colours && !weights) || count == 0) { return count; }
	FI_REQUIRE(capacity >= count, FI_ERR_INVALID, "room for %lld points, %lld voxels have a colour", static_cast<long long>(capacity),
	           static_cast<long long>(count));
	stage::Out<float> po(positions, 3 * count, memory);
	stage::Out<float> co(colours, v->channels * count, memory);
	stage::Out<float> we(weights, count, memory);
	hipLaunchKernelGGL(k_colour_gather, prim::grid(n), dim3(kThreads), 0, st, v->n[0], v->n[1], v->channels, v->max_weight, n, count,
	                   v->colour.as<float>(), v->colour_weight.as<float>(), flag, slot, po.dev, co.dev, we.dev);
	FI_HIP_TRY(hipGetLastError());
	po.back(st);
	co.back(st);
	we.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
	return count;
}

}  // namespace fi
