// fi_volume_pass.h -- one voxel-stationary pass over a depth volume, as the units that make one share it: the camera row and the
// table of a launch, the cull planes, the launch arguments, and steps 1 - 8 of include/fi_hip.h fi_volume_integrate for one
// voxel and one image.  fi_depth.hip (k_volume_integrate) and fi_colour.hip (k_colour_integrate) run this one body; what a
// kernel keeps per voxel beside tsdf and W is its own.  Everything here has internal linkage (the anonymous namespace is on
// purpose: the kernels of a unit name these types in their signatures, and each unit keeps its own), so only .hip units
// include it.
#pragma once

#include <cmath>
#include <cstring>
#include <vector>

#include "fi_depth.h"
#include "fi_solver_internal.h"

namespace fi {
namespace {

constexpr int kCams   = FI_DEPTH_CAMERAS;  // images one launch of a volume pass applies
constexpr int kPlanes = 5;                 // cull planes per image: behind, left, right, top, bottom
static_assert(kCams * kPlanes <= 64, "a wave evaluates every cull plane of a launch at once, a lane each");

struct CamRow {  // one image as the kernels read it
	float     r[12];  // rows of [R | t]
	float     fx, fy, cx, cy;
	int       width, height, kind, pad;
	long long off;    // the image's first pixel in the call's depths / incidences
	long long index;  // the image's index in the call (image_weights)
};

// the images of one launch and their cull planes: plane (s, k) is (n, o) over voxel coordinates; image s is skipped by a wave
// whose run of voxels has n . p + o < 0 everywhere for some k
struct CamTable {
	CamRow cam[kCams];
	float4 plane[kCams * kPlanes];
};

CamRow row_of(const fi_camera& c, long long off, long long index)
{
	CamRow r{};
	std::memcpy(r.r, c.pose, sizeof(r.r));
	r.fx     = c.fx;
	r.fy     = c.fy;
	r.cx     = c.cx;
	r.cy     = c.cy;
	r.width  = c.width;
	r.height = c.height;
	r.kind   = c.kind;
	r.off    = off;
	r.index  = index;
	return r;
}

__device__ __forceinline__ bool depth_ok(float d) { return d > 0.0f && d < INFINITY; }

struct VolArgs {
	int      nx, ny, nz;
	unsigned waves_x;  // waves along a row of x
	unsigned nwaves;   // waves_x * ny * nz
	float    truncation, max_weight;
};

VolArgs args_of(const fi_volume* v)
{
	VolArgs a{};
	a.nx = v->n[0];
	a.ny = v->n[1];
	a.nz = v->n[2];
	const int64_t waves_x = (v->n[0] + 63) / 64;
	const int64_t nwaves  = waves_x * v->n[1] * v->n[2];
	FI_REQUIRE(nwaves < (1LL << 31), FI_ERR_UNSUPPORTED, "%lld rows of 64 voxels in one volume", static_cast<long long>(nwaves));
	a.waves_x    = static_cast<unsigned>(waves_x);
	a.nwaves     = static_cast<unsigned>(nwaves);
	a.truncation = v->truncation;
	a.max_weight = v->max_weight;
	return a;
}

// The cull planes of one image over the voxels of v.  With c(p) = R p + t the camera point of voxel p, a form g = alpha . c(p)
// is linear in p.  The five forms: c_z (behind the camera where negative), and the four sides of the image widened by a pixel:
// fx c_x + (cx + 1) c_z < 0 is u < -1 for a voxel in front, and so on.  The kernel's own fp32 figures differ from the exact
// ones by a few 2^-24 of M = sum |alpha_a| (sum |R_aj| (size_j - 1) + |t_a|); the plane's offset is raised by 1e-5 M, forty
// times that, and the pixel of slack covers the rounding of u and v for pixel coordinates up to 2^16 (beyond: no cull).
void planes_of(const fi_camera& c, const fi_volume* v, bool cull, float4* out)
{
	for (int k = 0; k < kPlanes; ++k) { out[k] = float4{0.0f, 0.0f, 0.0f, 1.0f}; }  // (never negative: no cull)
	const double lim = 65536.0;
	if (!cull || std::fabs(c.cx) > lim || std::fabs(c.cy) > lim || c.width > lim || c.height > lim) { return; }
	const double alpha[kPlanes][3] = {{0.0, 0.0, 1.0},
	                                  {c.fx, 0.0, static_cast<double>(c.cx) + 1.0},
	                                  {-static_cast<double>(c.fx), 0.0, c.width + 1.0 - c.cx},
	                                  {0.0, c.fy, static_cast<double>(c.cy) + 1.0},
	                                  {0.0, -static_cast<double>(c.fy), c.height + 1.0 - c.cy}};
	for (int k = 0; k < kPlanes; ++k) {
		double n[3] = {0, 0, 0}, o = 0, M = 0;
		for (int a = 0; a < 3; ++a) {
			for (int j = 0; j < 3; ++j) {
				n[j] += alpha[k][a] * c.pose[4 * a + j];
				M += std::fabs(alpha[k][a] * c.pose[4 * a + j]) * (v->n[j] - 1);
			}
			o += alpha[k][a] * c.pose[4 * a + 3];
			M += std::fabs(alpha[k][a] * c.pose[4 * a + 3]);
		}
		const float4 p{static_cast<float>(n[0]), static_cast<float>(n[1]), static_cast<float>(n[2]),
		               std::nextafter(static_cast<float>(o + 1e-5 * M), INFINITY)};
		if (std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z) && std::isfinite(p.w)) { out[k] = p; }
	}
}

// the tables of a call's launches, kCams images each, in image order; *pixels receives the pixels of all m images
std::vector<CamTable> tables_of(const fi_volume* v, long m, const fi_camera* cameras, int64_t* pixels)
{
	const bool            cull = !test_switch("FI_NO_DEPTH_CULL");  // (the same bytes either way: tests/test_gpu_depth.py)
	const long            launches = (m + kCams - 1) / kCams;
	std::vector<CamTable> host(static_cast<size_t>(launches));
	std::memset(host.data(), 0, host.size() * sizeof(CamTable));
	*pixels = 0;
	for (long s = 0; s < m; ++s) {
		CamTable& t = host[static_cast<size_t>(s / kCams)];
		t.cam[s % kCams] = row_of(cameras[s], *pixels, s);
		planes_of(cameras[s], v, cull, t.plane + (s % kCams) * kPlanes);
		*pixels += camera_pixels(cameras[s]);
	}
	return host;
}

// ---- the device side: a wave owns 64 consecutive x of one (y, z) row, a thread one voxel ---------------------------------------
struct WaveRun {
	int x0, x1, y, z;  // the wave's voxels are (x0 .. x1, y, z)
};

__device__ __forceinline__ WaveRun run_of(const VolArgs& a, unsigned wid)
{
	const unsigned wx   = wid % a.waves_x;
	const unsigned rest = wid / a.waves_x;
	WaveRun        r;
	r.y  = static_cast<int>(rest % static_cast<unsigned>(a.ny));
	r.z  = static_cast<int>(rest / static_cast<unsigned>(a.ny));
	r.x0 = static_cast<int>(wx) * 64;
	r.x1 = min(r.x0 + 63, a.nx - 1);
	return r;
}

// The cull: lane s * kPlanes + k evaluates plane k of image s over the wave's run of voxels (a segment: the maximum of a linear
// form over it is its value at the middle plus |n_x| times the half length); bit s * kPlanes + k of the result is set where
// the plane excludes the whole run.  Every lane of the wave calls it.  The planes carry a margin (planes_of), so a skipped image
// is one every voxel of the run would have skipped by itself.
__device__ __forceinline__ unsigned long long culled_of(const CamTable* __restrict__ tab, int nc, const WaveRun& r, int lane)
{
	const float Y = static_cast<float>(r.y), Z = static_cast<float>(r.z);
	bool        excluded = false;
	if (lane < nc * kPlanes) {
		const float  h = 0.5f * static_cast<float>(r.x1 - r.x0);
		const float  mid = static_cast<float>(r.x0) + h;
		const float4 p = tab->plane[lane];
		excluded = (((p.x * mid + p.y * Y) + p.z * Z) + fabsf(p.x) * h) + p.w < 0.0f;
	}
	return __ballot(excluded);
}

__device__ __forceinline__ bool image_culled(unsigned long long culled, int s)
{
	return (culled >> (s * kPlanes)) & ((1ull << kPlanes) - 1);
}

// what image c says about voxel (X, Y, Z): steps 1 - 7
struct VoxelSample {
	float   g;    // (e q) / truncation, before the clamp
	float   f;    // min(g, 1)
	float   w;    // q image_weight
	int64_t pix;  // the pixel in the call's depths / incidences
};

// steps 1 - 7 of fi_volume_integrate; false: the image is skipped for this voxel
__device__ __forceinline__ bool voxel_sample(const VolArgs& a, const CamRow& c, float X, float Y, float Z, const float* __restrict__ depth,
                                             const float* __restrict__ inc, const float* __restrict__ iw, float min_inc, VoxelSample& o)
{
	const float cx = ((c.r[0] * X + c.r[1] * Y) + c.r[2] * Z) + c.r[3];
	const float cy = ((c.r[4] * X + c.r[5] * Y) + c.r[6] * Z) + c.r[7];
	const float cz = ((c.r[8] * X + c.r[9] * Y) + c.r[10] * Z) + c.r[11];
	if (!(cz > 0.0f)) { return false; }
	const float fu = floorf(c.fx * (cx / cz) + c.cx);
	const float fv = floorf(c.fy * (cy / cz) + c.cy);
	if (!(fu >= 0.0f && fu < 2147483648.0f && fv >= 0.0f && fv < 2147483648.0f)) { return false; }
	const int col = static_cast<int>(fu), row = static_cast<int>(fv);
	if (col >= c.width || row >= c.height) { return false; }
	o.pix         = c.off + static_cast<int64_t>(row) * c.width + col;
	const float d = depth[o.pix];
	if (!depth_ok(d)) { return false; }
	const float r = c.kind == FI_DEPTH_Z ? cz : sqrtf((cx * cx + cy * cy) + cz * cz);
	const float e = d - r;
	if (e < -a.truncation) { return false; }
	float q = 1.0f;
	if (inc) {
		q = inc[o.pix];
		if (!(q >= min_inc && fabsf(q) < INFINITY)) { return false; }
	}
	o.g = (e * q) / a.truncation;
	o.f = o.g < 1.0f ? o.g : 1.0f;
	o.w = q * (iw ? iw[c.index] : 1.0f);
	return o.w > 0.0f;
}

// step 8
__device__ __forceinline__ void voxel_fuse(const VolArgs& a, const VoxelSample& s, float& t, float& W)
{
	const float sum = W + s.w;
	t = (t * W + s.f * s.w) / sum;
	W = sum < a.max_weight ? sum : a.max_weight;
}

}  // namespace
}  // namespace fi
