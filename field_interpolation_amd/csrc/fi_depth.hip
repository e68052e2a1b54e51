// fi_depth.hip -- depth images on the device.  Two things: a depth image unprojected into oriented points (a thread per pixel:
// the image's own neighbourhood gives the normal, the known viewpoint its sign), and a truncated signed distance volume over a
// 3-D lattice (a thread per voxel: the voxel is projected into every image and averages what it sees).  The contract is
// include/fi_hip.h (fi_depth_unproject, fi_volume_integrate), tests/depth_reference.py its definition in numpy; DESIGN.md 4.27.
// All arithmetic is fp32, one rounding per operation (the tree's -ffp-contract=off), and nothing is accumulated by atomics:
// a voxel's images are applied by its own thread in image order, so a repeated call gives the same bytes.
#include "fi_depth.h"

#include <cmath>
#include <cstring>

#include "fi_prim.h"
#include "fi_solver_internal.h"
#include "fi_stage.h"
#include "fi_volume_pass.h"

namespace fi {
namespace {

// (the camera row, the table of a launch, the cull planes and steps 1 - 8 of a voxel: fi_volume_pass.h, shared with fi_colour.hip)

// ---- a depth image becomes oriented points ---------------------------------------------------------------------------------
struct Vec3 {
	float x, y, z;
};

// the camera point of pixel (row, col) at depth d
__device__ __forceinline__ Vec3 camera_point(const CamRow& c, int row, int col, float d)
{
	const float px = ((static_cast<float>(col) + 0.5f) - c.cx) / c.fx;
	const float py = ((static_cast<float>(row) + 0.5f) - c.cy) / c.fy;
	if (c.kind == FI_DEPTH_Z) { return Vec3{px * d, py * d, d}; }
	const float l = sqrtf((px * px + py * py) + 1.0f);
	return Vec3{(px / l) * d, (py / l) * d, (1.0f / l) * d};
}

// R^T e
__device__ __forceinline__ Vec3 rotate_back(const CamRow& c, Vec3 e)
{
	return Vec3{(c.r[0] * e.x + c.r[4] * e.y) + c.r[8] * e.z, (c.r[1] * e.x + c.r[5] * e.y) + c.r[9] * e.z,
	            (c.r[2] * e.x + c.r[6] * e.y) + c.r[10] * e.z};
}

__device__ __forceinline__ Vec3 world_point(const CamRow& c, int row, int col, float d)
{
	const Vec3 p = camera_point(c, row, col, d);
	return rotate_back(c, Vec3{p.x - c.r[3], p.y - c.r[7], p.z - c.r[11]});
}

// the difference of the world points of the neighbours after and before pixel (row, col) along one image axis: central where
// both qualify, one-sided with the one that does; false: neither qualifies
__device__ __forceinline__ bool difference(const CamRow& c, const float* __restrict__ depth, int row, int col, int drow, int dcol, float d,
                                           Vec3 here, float max_jump, Vec3& out)
{
	const int  rb = row - drow, cb = col - dcol, ra = row + drow, ca = col + dcol;
	const bool in_b = rb >= 0 && cb >= 0, in_a = ra < c.height && ca < c.width;
	const float db = in_b ? depth[static_cast<int64_t>(rb) * c.width + cb] : 0.0f;
	const float da = in_a ? depth[static_cast<int64_t>(ra) * c.width + ca] : 0.0f;
	const bool ok_b = in_b && depth_ok(db) && fabsf(db - d) <= max_jump;
	const bool ok_a = in_a && depth_ok(da) && fabsf(da - d) <= max_jump;
	if (!ok_a && !ok_b) { return false; }
	const Vec3 after  = ok_a ? world_point(c, ra, ca, da) : here;
	const Vec3 before = ok_b ? world_point(c, rb, cb, db) : here;
	out = Vec3{after.x - before.x, after.y - before.y, after.z - before.z};
	return true;
}

__global__ __launch_bounds__(kThreads) void k_depth_unproject(CamRow c, int64_t npix, const float* __restrict__ depth, float max_jump,
                                                               float* __restrict__ positions, float* __restrict__ normals,
                                                               float* __restrict__ incidence, unsigned char* __restrict__ valid)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= npix) { return; }
	const int   row = static_cast<int>(i / c.width), col = static_cast<int>(i % c.width);
	const float d   = depth[i];
	const bool  ok  = depth_ok(d);
	Vec3        p{NAN, NAN, NAN}, n{0.0f, 0.0f, 0.0f};
	float       q = 0.0f;
	if (ok) {
		p = world_point(c, row, col, d);
		Vec3 a, b;
		if ((normals || incidence) && difference(c, depth, row, col, 0, 1, d, p, max_jump, a) &&
		    difference(c, depth, row, col, 1, 0, d, p, max_jump, b)) {
			Vec3        m{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
			const float len = sqrtf((m.x * m.x + m.y * m.y) + m.z * m.z);
			m = Vec3{m.x / len, m.y / len, m.z / len};
			const Vec3  v  = rotate_back(c, camera_point(c, row, col, d));  // from the eye to the point
			const float lv = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
			float       s  = (m.x * (v.x / lv) + m.y * (v.y / lv)) + m.z * (v.z / lv);
			if (s > 0.0f) {  // it points away from the eye
				m = Vec3{-m.x, -m.y, -m.z};
				s = -s;
			}
			float t = -s;
			t       = t < 1.0f ? t : 1.0f;
			if (len > 0.0f && len < INFINITY && t > 0.0f) {
				n = m;
				q = t;
			}
		}
	}
	if (positions) {
		positions[3 * i + 0] = p.x;
		positions[3 * i + 1] = p.y;
		positions[3 * i + 2] = p.z;
	}
	if (normals) {
		normals[3 * i + 0] = n.x;
		normals[3 * i + 1] = n.y;
		normals[3 * i + 2] = n.z;
	}
	if (incidence) { incidence[i] = q; }
	if (valid) { valid[i] = ok ? 1 : 0; }
}

// ---- the volume -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_volume_fill(int64_t n, float* __restrict__ tsdf, float* __restrict__ weight)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n) { return; }
	tsdf[i]   = 1.0f;
	weight[i] = 0.0f;
}

// Voxel-stationary fusion: a wave owns 64 consecutive x of one (y, z) row, a thread one voxel.  The voxel's tsdf and weight are
// read once, up to kCams images are applied in image order, and both are written once.  The images' cameras come from a table
// indexed by the (wave-uniform) loop counter: scalar loads into scalar registers.  Depth and incidence are gathered: a wave's
// voxels project onto a short run of pixels.  An image with a cull plane that excludes the wave's whole run is skipped by the
// whole wave.  The run, the cull and the steps of one image are fi_volume_pass.h's.  No LDS, no atomics.
__global__ __launch_bounds__(kThreads) void k_volume_integrate(VolArgs a, const CamTable* __restrict__ tab, int nc,
                                                                const float* __restrict__ depth, const float* __restrict__ inc,
                                                                const float* __restrict__ iw, float min_inc, float* __restrict__ tsdf,
                                                                float* __restrict__ weight)
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
	float         t = tsdf[idx], W = weight[idx];
	for (int s = 0; s < nc; ++s) {
		if (image_culled(culled, s)) { continue; }
		VoxelSample v;
		if (!voxel_sample(a, tab->cam[s], X, Y, Z, depth, inc, iw, min_inc, v)) { continue; }
		voxel_fuse(a, v, t, W);
	}
	tsdf[idx]   = t;
	weight[idx] = W;
}

// ---- the band as data points ---------------------------------------------------------------------------------------------------
// flag[i] = 1 for a voxel of the band, flag[n] = 0: the exclusive sums' last entry is the count
__global__ __launch_bounds__(kThreads) void k_volume_mark(int64_t n, const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                           float min_weight, uint32_t* __restrict__ flag)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i > n) { return; }
	uint32_t f = 0;
	if (i < n) {
		const float W = weight[i];
		f = (W >= min_weight && W > 0.0f && fabsf(tsdf[i]) < 1.0f) ? 1u : 0u;
	}
	flag[i] = f;
}

__global__ __launch_bounds__(kThreads) void k_volume_gather(VolArgs a, int64_t n, int64_t capacity, const float* __restrict__ tsdf,
                                                             const float* __restrict__ weight, const uint32_t* __restrict__ flag,
                                                             const uint32_t* __restrict__ slot, float* __restrict__ positions,
                                                             float* __restrict__ values, float* __restrict__ weights)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (i >= n || !flag[i]) { return; }
	const int64_t o = slot[i];
	if (o >= capacity) { return; }
	if (positions) {
		const int64_t plane = static_cast<int64_t>(a.nx) * a.ny;
		const int64_t in_plane = i % plane;
		positions[3 * o + 0] = static_cast<float>(in_plane % a.nx);
		positions[3 * o + 1] = static_cast<float>(in_plane / a.nx);
		positions[3 * o + 2] = static_cast<float>(i / plane);
	}
	if (values) { values[o] = tsdf[i] * a.truncation; }
	if (weights) { weights[o] = weight[i] / a.max_weight; }
}

// flags and their exclusive sums over the volume's voxels, as pieces of `block`; returns the count
int64_t mark_band(const fi_volume* v, float min_weight, DevBuf& block, uint32_t*& flag, uint32_t*& slot, hipStream_t st)
{
	const int64_t n = v->nvox;
	prim::Scratch tmp;
	prim::arena_alloc(block, [&](prim::Arena& ar) {
		flag      = ar.take<uint32_t>(n + 1);
		slot      = ar.take<uint32_t>(n + 1);
		tmp.bytes = prim::scan_bytes(n + 1);
		tmp.p     = ar.take<char>(static_cast<int64_t>(tmp.bytes));
	});
	hipLaunchKernelGGL(k_volume_mark, prim::grid(n + 1), dim3(kThreads), 0, st, n, v->tsdf.as<float>(), v->weight.as<float>(), min_weight, flag);
	FI_HIP_TRY(hipGetLastError());
	prim::scan_u32(flag, slot, n + 1, tmp, st);
	return prim::read_u32(slot + n, st);
}

}  // namespace

int64_t camera_pixels(const fi_camera& cam) { return static_cast<int64_t>(cam.width) * cam.height; }

void check_camera(const fi_camera& cam)
{
	FI_REQUIRE(cam.kind == FI_DEPTH_Z || cam.kind == FI_DEPTH_RANGE, FI_ERR_INVALID, "bad depth kind %d", cam.kind);
	FI_REQUIRE(cam.width >= 1 && cam.height >= 1, FI_ERR_INVALID, "a %d x %d image", cam.width, cam.height);
	for (int i = 0; i < 12; ++i) { FI_REQUIRE(std::isfinite(cam.pose[i]), FI_ERR_INVALID, "pose[%d] is not finite", i); }
	FI_REQUIRE(cam.fx > 0.0f && cam.fy > 0.0f && std::isfinite(cam.fx) && std::isfinite(cam.fy), FI_ERR_INVALID,
	           "fx and fy must be > 0 and finite (got %g, %g)", static_cast<double>(cam.fx), static_cast<double>(cam.fy));
	FI_REQUIRE(std::isfinite(cam.cx) && std::isfinite(cam.cy), FI_ERR_INVALID, "cx or cy is not finite");
}

void depth_unproject(const fi_camera& cam, const float* depth, float max_jump, float* positions, float* normals, float* incidence,
                     unsigned char* valid, int memory, hipStream_t st)
{
	const int64_t             n = camera_pixels(cam);
	AllocStream               alloc_on(st);
	stage::In<float>          d(depth, n, memory, st);
	stage::Out<float>         po(positions, 3 * n, memory);
	stage::Out<float>         nr(normals, 3 * n, memory);
	stage::Out<float>         in(incidence, n, memory);
	stage::Out<unsigned char> va(valid, n, memory);
	hipLaunchKernelGGL(k_depth_unproject, prim::grid(n), dim3(kThreads), 0, st, row_of(cam, 0, 0), n, d.dev, max_jump, po.dev, nr.dev, in.dev,
	                   va.dev);
	FI_HIP_TRY(hipGetLastError());
	po.back(st);
	nr.back(st);
	in.back(st);
	va.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
}

void volume_reset(fi_volume* v, hipStream_t st)
{
	hipLaunchKernelGGL(k_volume_fill, prim::grid(v->nvox), dim3(kThreads), 0, st, v->nvox, v->tsdf.as<float>(), v->weight.as<float>());
	FI_HIP_TRY(hipGetLastError());
	FI_HIP_TRY(hipStreamSynchronize(st));
}

void volume_integrate(fi_volume* v, long m, const fi_camera* cameras, const float* depths, const float* incidences,
                      const float* image_weights, float min_incidence, int memory, hipStream_t st)
{
	if (m == 0) { return; }
	const VolArgs               a = args_of(v);
	int64_t                     pixels = 0;
	const std::vector<CamTable> host = tables_of(v, m, cameras, &pixels);
	const long                  launches = static_cast<long>(host.size());
	AllocStream     alloc_on(st);
	const float *   d = nullptr, *q = nullptr, *iw = nullptr;
	const CamTable* tab = nullptr;
	DevBuf          block;
	prim::arena_alloc(block, [&](prim::Arena& ar) {
		tab = stage::in(ar, host.data(), launches, FI_HOST, st);
		d   = stage::in(ar, depths, pixels, memory, st);
		q   = stage::in(ar, incidences, pixels, memory, st);
		iw  = stage::in(ar, image_weights, m, memory, st);
	});
	const dim3 grid((a.nwaves + kThreads / 64 - 1) / (kThreads / 64));
	for (long l = 0; l < launches; ++l) {
		const int nc = static_cast<int>(std::min<long>(kCams, m - l * kCams));
		hipLaunchKernelGGL(k_volume_integrate, grid, dim3(kThreads), 0, st, a, tab + l, nc, d, q, iw, min_incidence, v->tsdf.as<float>(),
		                   v->weight.as<float>());
		FI_HIP_TRY(hipGetLastError());
	}
	FI_HIP_TRY(hipStreamSynchronize(st));  // (the table and the staged images live until here)
}

int64_t volume_constraints(const fi_volume* v, float min_weight, int64_t capacity, float* positions, float* values, float* weights,
                           int memory, hipStream_t st)
{
	AllocStream   alloc_on(st);
	DevBuf        block;
	uint32_t *    flag = nullptr, *slot = nullptr;
	const int64_t count = mark_band(v, min_weight, block, flag, slot, st);
	if ((!positions && !values && !weights) || count == 0) { return count; }
	FI_REQUIRE(capacity >= count, FI_ERR_INVALID, "room for %lld points, the band holds %lld", static_cast<long long>(capacity),
	           static_cast<long long>(count));
	stage::Out<float> po(positions, 3 * count, memory);
	stage::Out<float> va(values, count, memory);
	stage::Out<float> we(weights, count, memory);
	hipLaunchKernelGGL(k_volume_gather, prim::grid(v->nvox), dim3(kThreads), 0, st, args_of(v), v->nvox, count, v->tsdf.as<float>(),
	                   v->weight.as<float>(), flag, slot, po.dev, va.dev, we.dev);
	FI_HIP_TRY(hipGetLastError());
	po.back(st);
	va.back(st);
	we.back(st);
	FI_HIP_TRY(hipStreamSynchronize(st));
	return count;
}

int64_t volume_constraints_device(const fi_volume* v, float min_weight, DevBuf& positions, DevBuf& values, DevBuf& weights,
                                  hipStream_t st)
{
	AllocStream   alloc_on(st);
	DevBuf        block;
	uint32_t *    flag = nullptr, *slot = nullptr;
	const int64_t count = mark_band(v, min_weight, block, flag, slot, st);
	if (count == 0) { return 0; }
	positions.alloc(sizeof(float) * 3 * count);
	values.alloc(sizeof(float) * count);
	weights.alloc(sizeof(float) * count);
	hipLaunchKernelGGL(k_volume_gather, prim::grid(v->nvox), dim3(kThreads), 0, st, args_of(v), v->nvox, count, v->tsdf.as<float>(),
	                   v->weight.as<float>(), flag, slot, positions.as<float>(), values.as<float>(), weights.as<float>());
	FI_HIP_TRY(hipGetLastError());
	FI_HIP_TRY(hipStreamSynchronize(st));
	return count;
}

}  // namespace fi
