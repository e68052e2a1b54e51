// The depth calls of the C++ drop-in against the C ABI.
//   test_depth <views.bin> <out.bin>   views.bin: int32 m, then per view 12 pose floats, fx, fy, cx, cy, int32 width, height,
//                                      range (1 / 0), then the m depth images back to back, for a 20 x 18 x 16 lattice.
//                                      depth_to_points, DepthVolume and GpuLatticeField::add_volume are called on them and
//                                      held to the C ABI's bytes, with host and with device pointers.
//                                      out.bin: positions, normals, incidence, valid of view 0; tsdf, weight; the constraints'
//                                      positions, values, weights; int64 counts in front
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include <fi_hip.h>

#include <field_interpolation/gpu_field.hpp>

namespace fi = field_interpolation;

static void require(bool ok, const char* what)
{
	if (!ok) {
		std::printf("FAILED: %s (%s)\n", what, fi_last_error());
		std::exit(1);
	}
	std::printf("ok   %s\n", what);
}

template <typename T>
static void put(std::FILE* f, const std::vector<T>& v)
{
	const long long n = static_cast<long long>(v.size());
	std::fwrite(&n, sizeof(n), 1, f);
	if (n) { std::fwrite(v.data(), sizeof(T), v.size(), f); }
}

template <typename T>
static bool same(const std::vector<T>& a, const std::vector<T>& b)
{
	return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

template <typename T>
static T* on_device(const std::vector<T>& v)
{
	T* d = nullptr;
	require(hipMalloc(reinterpret_cast<void**>(&d), (v.size() + 1) * sizeof(T)) == hipSuccess &&
	            hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess,
	        "upload");
	return d;
}

template <typename T>
static std::vector<T> from_device(const T* d, size_t count)
{
	std::vector<T> v(count);
	require(hipMemcpy(v.data(), d, count * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess, "download");
	return v;
}

int main(int argc, char** argv)
{
	require(argc == 3, "usage: test_depth <views.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open views");
	int m = 0;
	require(std::fread(&m, sizeof(m), 1, in) == 1 && m > 0, "read view count");
	std::vector<fi::DepthCamera> cams(m);
	std::vector<fi_camera>       ccams(m);
	size_t                       pixels = 0;
	for (int s = 0; s < m; ++s) {
		fi::DepthCamera& c = cams[s];
		int              range = 0;
		require(std::fread(c.pose, sizeof(float), 12, in) == 12 && std::fread(&c.fx, sizeof(float), 1, in) == 1 &&
		            std::fread(&c.fy, sizeof(float), 1, in) == 1 && std::fread(&c.cx, sizeof(float), 1, in) == 1 &&
		            std::fread(&c.cy, sizeof(float), 1, in) == 1 && std::fread(&c.width, sizeof(int), 1, in) == 1 &&
		            std::fread(&c.height, sizeof(int), 1, in) == 1 && std::fread(&range, sizeof(int), 1, in) == 1,
		        "read a camera");
		c.range = range != 0;
		std::memcpy(ccams[s].pose, c.pose, sizeof(c.pose));
		ccams[s].fx = c.fx, ccams[s].fy = c.fy, ccams[s].cx = c.cx, ccams[s].cy = c.cy;
		ccams[s].width = c.width, ccams[s].height = c.height, ccams[s].kind = c.range ? FI_DEPTH_RANGE : FI_DEPTH_Z;
		pixels += static_cast<size_t>(c.width) * c.height;
	}
	std::vector<float> depths(pixels);
	require(std::fread(depths.data(), sizeof(float), pixels, in) == pixels, "read the images");
	std::fclose(in);

	// one image as oriented points
	const size_t               n0 = static_cast<size_t>(cams[0].width) * cams[0].height;
	const std::vector<float>   first(depths.begin(), depths.begin() + n0);
	std::vector<float>         p, nr, inc, p2(3 * n0), nr2(3 * n0), inc2(n0);
	std::vector<unsigned char> va, va2(n0);
	require(fi::depth_to_points(cams[0], first, &p, &nr, &inc, &va, 1.0f) && va.size() == n0, "depth_to_points");
	require(fi_depth_unproject(&ccams[0], first.data(), 1.0f, p2.data(), nr2.data(), inc2.data(), va2.data(), FI_HOST) == FI_OK && same(p, p2) &&
	            same(nr, nr2) && same(inc, inc2) && same(va, va2),
	        "... = fi_depth_unproject");
	std::vector<float> only;
	require(fi::depth_to_points(cams[0], first, nullptr, nullptr, &only, nullptr, 1.0f) && same(only, inc), "... the incidence alone");
	require(!fi::depth_to_points(cams[0], first, nullptr) && !fi::depth_to_points(cams[0], depths, &only) &&
	            !fi::depth_to_points(cams[0], first, &only, nullptr, nullptr, nullptr, -1.0f),
	        "... no output, a wrong image size, a negative jump are refused");
	float*         dd = on_device(first);
	float*         dp = on_device(p2);
	float*         dn = on_device(nr2);
	float*         di = on_device(inc2);
	unsigned char* dv = on_device(va2);
	require(fi_depth_unproject(&ccams[0], dd, 1.0f, dp, dn, di, dv, FI_DEVICE) == FI_OK && same(from_device(dp, p.size()), p) &&
	            same(from_device(dn, nr.size()), nr) && same(from_device(di, inc.size()), inc) && same(from_device(dv, va.size()), va),
	        "device pointers: fi_depth_unproject");
	hipFree(dd), hipFree(dp), hipFree(dn), hipFree(di), hipFree(dv);

	// the volume
	const std::vector<int> sizes = {20, 18, 16};
	const size_t           nvox  = 20 * 18 * 16;
	fi::DepthVolume        volume(sizes, 2.5f, 4.0f);
	require(volume.valid() && volume.num_voxels() == nvox, "DepthVolume");
	require(volume.integrate(cams, depths), "integrate");
	std::vector<float> tsdf, weight, tsdf2(nvox), weight2(nvox);
	require(volume.copy(&tsdf, &weight) && tsdf.size() == nvox, "copy");
	fi_volume* raw = nullptr;
	require(fi_volume_create(&raw, 3, sizes.data(), 2.5f, 4.0f) == FI_OK &&
	            fi_volume_integrate(raw, m, ccams.data(), depths.data(), nullptr, nullptr, 0.5f, FI_HOST) == FI_OK &&
	            fi_volume_copy(raw, tsdf2.data(), weight2.data(), FI_HOST) == FI_OK && same(tsdf, tsdf2) && same(weight, weight2),
	        "... = fi_volume_integrate");
	float* ddep = on_device(depths);
	float* dt   = on_device(tsdf2);
	float* dw   = on_device(weight2);
	fi_volume* raw2 = nullptr;
	require(fi_volume_create(&raw2, 3, sizes.data(), 2.5f, 4.0f) == FI_OK &&
	            fi_volume_integrate(raw2, m, ccams.data(), ddep, nullptr, nullptr, 0.5f, FI_DEVICE) == FI_OK &&
	            fi_volume_copy(raw2, dt, dw, FI_DEVICE) == FI_OK && same(from_device(dt, nvox), tsdf) && same(from_device(dw, nvox), weight),
	        "device pointers: fi_volume_integrate, fi_volume_copy");
	fi::DepthVolume resumed(sizes, 2.5f, 4.0f);
	std::vector<float> t3, w3;
	require(resumed.load(tsdf, weight) && resumed.copy(&t3, &w3) && same(t3, tsdf) && same(w3, weight), "load");
	require(fi_volume_load(raw2, dt, dw, FI_DEVICE) == FI_OK && fi_volume_copy(raw2, tsdf2.data(), nullptr, FI_HOST) == FI_OK && same(tsdf2, tsdf),
	        "device pointers: fi_volume_load");
	hipFree(ddep), hipFree(dt), hipFree(dw);
	long seen = 0;
	for (float w : weight) { seen += w > 0.0f; }
	require(seen > 100, "... the images reach the lattice");
	require(!volume.integrate(cams, first) && !resumed.load(first, weight) && !fi::DepthVolume(std::vector<int>{8, 8}, 1.0f).valid() &&
	            !fi::DepthVolume(sizes, 0.0f).valid(),
	        "... a short image list, a short state, a 2-D lattice, a zero truncation are refused");

	// the band
	std::vector<float> cp, cv, cw;
	require(volume.constraints(&cp, &cv, &cw, 1.0f) && cp.size() == 3 * cv.size() && cv.size() == cw.size() && !cv.empty(), "constraints");
	long               count = 0;
	require(fi_volume_constraints(raw, 1.0f, &count, nullptr, nullptr, nullptr, FI_HOST) == FI_OK && count == static_cast<long>(cv.size()),
	        "... the count of fi_volume_constraints");
	std::vector<float> cp2(3 * count), cv2(count), cw2(count);
	require(fi_volume_constraints(raw, 1.0f, &count, cp2.data(), cv2.data(), cw2.data(), FI_HOST) == FI_OK && same(cp, cp2) && same(cv, cv2) &&
	            same(cw, cw2),
	        "... = fi_volume_constraints");
	float* dcp = on_device(cp2);
	float* dcv = on_device(cv2);
	float* dcw = on_device(cw2);
	require(fi_volume_constraints(raw, 1.0f, &count, dcp, dcv, dcw, FI_DEVICE) == FI_OK && same(from_device(dcp, cp.size()), cp) &&
	            same(from_device(dcv, cv.size()), cv) && same(from_device(dcw, cw.size()), cw),
	        "device pointers: fi_volume_constraints");
	hipFree(dcp), hipFree(dcv), hipFree(dcw);

	// into a field
	fi::GpuLatticeField field(sizes);
	field.add_field_constraints(fi::Weights());
	require(field.add_volume(volume, 0.7f, fi::ValueKernel::kNearestNeighbor, 1.0f), "add_volume");
	// (the rows are counted when the field is assembled, which a solve does)
	require(field.solve_with_guess(std::vector<float>(nvox, 0.0f), 20, 1e-3f).size() == nvox && field.num_data_rows() == cv.size(),
	        "... every voxel of the band is a data row of the field");
	fi::GpuLatticeField other(sizes);
	require(!other.add_volume(fi::DepthVolume(std::vector<int>{20, 18, 15}, 1.0f), 1.0f), "... a volume of other sizes is refused");
	fi_volume_destroy(raw);
	fi_volume_destroy(raw2);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, p);
	put(out, nr);
	put(out, inc);
	put(out, va);
	put(out, tsdf);
	put(out, weight);
	put(out, cp);
	put(out, cv);
	put(out, cw);
	std::fclose(out);
	std::printf("all depth checks passed\n");
	return 0;
}
