// The colour calls of the C++ drop-in against the C ABI.
//   test_colour <views.bin> <out.bin>   views.bin: int32 m, then per view 12 pose floats, fx, fy, cx, cy, int32 width, height,
//                                       range (1 / 0), then the m depth images back to back, then their colour images (3
//                                       channels, pixel-interleaved), then int32 n and n query points (3 floats each), for a
//                                       20 x 18 x 16 lattice.  The last view is also the one that renders.  The colour members
//                                       of DepthVolume are called on them and held to the C ABI's bytes, with host and with
//                                       device pointers.
//                                       out.bin: tsdf, weight, colours, colour weight; the samples and their flags; the
//                                       image's depth and colours; the constraints' positions, colours, weights; int64 counts
//                                       in front
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
	require(argc == 3, "usage: test_colour <views.bin> <out.bin>");
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
	const int          C = 3;
	std::vector<float> depths(pixels), colours(C * pixels);
	require(std::fread(depths.data(), sizeof(float), pixels, in) == pixels, "read the depth images");
	require(std::fread(colours.data(), sizeof(float), C * pixels, in) == C * pixels, "read the colour images");
	int n = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "read the point count");
	std::vector<float> points(3 * static_cast<size_t>(n));
	require(std::fread(points.data(), sizeof(float), points.size(), in) == points.size(), "read the points");
	std::fclose(in);

	// fusion
	const std::vector<int> sizes = {20, 18, 16};
	const size_t           nvox  = 20 * 18 * 16;
	fi::DepthVolume        volume(sizes, 2.5f, 4.0f);
	require(volume.valid() && volume.channels() == 0, "DepthVolume");
	std::vector<float> none;
	require(!volume.integrate_colour(cams, depths, colours) && !volume.copy_colours(&none, nullptr) && !volume.sample_colours(points, &none),
	        "... without channels the colour calls are refused");
	require(!volume.set_channels(0) && !volume.set_channels(5) && volume.set_channels(C) && volume.channels() == C && !volume.set_channels(C),
	        "set_channels");
	require(volume.integrate_colour(cams, depths, colours), "integrate_colour");
	std::vector<float> tsdf, weight, col, cw;
	require(volume.copy(&tsdf, &weight) && volume.copy_colours(&col, &cw) && col.size() == C * nvox && cw.size() == nvox, "copy_colours");
	fi::DepthVolume plain(sizes, 2.5f, 4.0f);
	std::vector<float> t2, w2;
	require(plain.integrate(cams, depths) && plain.copy(&t2, &w2) && same(tsdf, t2) && same(weight, w2), "... tsdf and weight = integrate");
	fi_volume*         raw = nullptr;
	std::vector<float> col2(C * nvox), cw2(nvox);
	require(fi_volume_create(&raw, 3, sizes.data(), 2.5f, 4.0f) == FI_OK && fi_volume_set_channels(raw, C) == FI_OK &&
	            fi_volume_integrate_colour(raw, m, ccams.data(), depths.data(), nullptr, nullptr, 0.5f, colours.data(), 1.0f, FI_HOST) == FI_OK &&
	            fi_volume_colour_copy(raw, col2.data(), cw2.data(), FI_HOST) == FI_OK && same(col, col2) && same(cw, cw2),
	        "... = fi_volume_integrate_colour");
	float*     ddep = on_device(depths);
	float*     dcol = on_device(colours);
	float*     da   = on_device(col2);
	float*     dw   = on_device(cw2);
	fi_volume* raw2 = nullptr;
	require(fi_volume_create(&raw2, 3, sizes.data(), 2.5f, 4.0f) == FI_OK && fi_volume_set_channels(raw2, C) == FI_OK &&
	            fi_volume_integrate_colour(raw2, m, ccams.data(), ddep, nullptr, nullptr, 0.5f, dcol, 1.0f, FI_DEVICE) == FI_OK &&
	            fi_volume_colour_copy(raw2, da, dw, FI_DEVICE) == FI_OK && same(from_device(da, C * nvox), col) && same(from_device(dw, nvox), cw),
	        "device pointers: fi_volume_integrate_colour, fi_volume_colour_copy");
	fi::DepthVolume    resumed(sizes, 2.5f, 4.0f);
	std::vector<float> a3, w3;
	require(resumed.set_channels(C) && resumed.load(tsdf, weight) && resumed.load_colours(col, cw) && resumed.copy_colours(&a3, &w3) &&
	            same(a3, col) && same(w3, cw),
	        "load_colours");
	require(fi_volume_colour_load(raw2, da, dw, FI_DEVICE) == FI_OK && fi_volume_colour_copy(raw2, col2.data(), nullptr, FI_HOST) == FI_OK &&
	            same(col2, col),
	        "device pointers: fi_volume_colour_load");
	hipFree(ddep), hipFree(dcol), hipFree(da), hipFree(dw);
	long seen = 0;
	for (float w : cw) { seen += w > 0.0f; }
	require(seen > 100, "... the images colour the lattice");
	require(!volume.integrate_colour(cams, depths, depths) && !resumed.load_colours(tsdf, cw) &&
	            !volume.integrate_colour(cams, depths, colours, std::vector<float>(), std::vector<float>(), 0.5f, 0.0f),
	        "... a short colour list, a short state, a zero band are refused");

	// samples
	std::vector<float>         sc, sc2(static_cast<size_t>(C) * n);
	std::vector<unsigned char> sv, sv2(n);
	require(volume.sample_colours(points, &sc, &sv, 0.5f) && sc.size() == static_cast<size_t>(C) * n && sv.size() == static_cast<size_t>(n),
	        "sample_colours");
	require(fi_volume_colour_sample(raw, 0.5f, n, points.data(), sc2.data(), sv2.data(), FI_HOST) == FI_OK && same(sc, sc2) && same(sv, sv2),
	        "... = fi_volume_colour_sample");
	float*         dpts = on_device(points);
	float*         dsc  = on_device(sc2);
	unsigned char* dsv  = on_device(sv2);
	require(fi_volume_colour_sample(raw, 0.5f, n, dpts, dsc, dsv, FI_DEVICE) == FI_OK && same(from_device(dsc, sc.size()), sc) &&
	            same(from_device(dsv, sv.size()), sv),
	        "device pointers: fi_volume_colour_sample");
	hipFree(dpts), hipFree(dsc), hipFree(dsv);
	std::vector<float> alone;
	require(volume.sample_colours(points, &alone, nullptr, 0.5f) && same(alone, sc) && !volume.sample_colours(points, nullptr),
	        "... the colours alone; no output is refused");

	// an image
	const fi::DepthCamera& view = cams[m - 1];
	const size_t           P    = static_cast<size_t>(view.width) * view.height;
	std::vector<float>     depth, image, pos, plain_depth, plain_pos, depth2(P), image2(C * P);
	require(volume.render_colour(view, &depth, &image, fi::MarchOptions(), 0.5f, &pos) && depth.size() == P && image.size() == C * P &&
	            pos.size() == 3 * P,
	        "render_colour");
	require(volume.render(view, &plain_depth, fi::MarchOptions(), &plain_pos) && same(depth, plain_depth) && same(pos, plain_pos),
	        "... depth and positions = render");
	fi_march_options opt;
	require(fi_march_default_options(&opt) == FI_OK &&
	            fi_volume_render_colour(raw, &opt, &ccams[m - 1], 0.5f, depth2.data(), nullptr, nullptr, nullptr, image2.data(), FI_HOST) == FI_OK &&
	            same(depth, depth2) && same(image, image2),
	        "... = fi_volume_render_colour");
	float* dd = on_device(depth2);
	float* di = on_device(image2);
	require(fi_volume_render_colour(raw, &opt, &ccams[m - 1], 0.5f, dd, nullptr, nullptr, nullptr, di, FI_DEVICE) == FI_OK &&
	            same(from_device(dd, P), depth) && same(from_device(di, C * P), image),
	        "device pointers: fi_volume_render_colour");
	hipFree(dd), hipFree(di);
	long hits = 0;
	for (float d : depth) { hits += std::isfinite(d); }
	require(hits > 20 && !volume.render_colour(view, &depth, nullptr), "... the image meets the surface; no colour output is refused");

	// the coloured voxels
	std::vector<float> cp, cc, cwt;
	require(volume.colour_constraints(&cp, &cc, &cwt, 1.0f) && cp.size() == 3 * cwt.size() && cc.size() == C * cwt.size() && !cwt.empty(),
	        "colour_constraints");
	long count = 0;
	require(fi_volume_colour_constraints(raw, 1.0f, &count, nullptr, nullptr, nullptr, FI_HOST) == FI_OK && count == static_cast<long>(cwt.size()),
	        "... the count of fi_volume_colour_constraints");
	std::vector<float> cp2(3 * count), cc2(C * count), cwt2(count);
	require(fi_volume_colour_constraints(raw, 1.0f, &count, cp2.data(), cc2.data(), cwt2.data(), FI_HOST) == FI_OK && same(cp, cp2) &&
	            same(cc, cc2) && same(cwt, cwt2),
	        "... = fi_volume_colour_constraints");
	float* dcp = on_device(cp2);
	float* dcc = on_device(cc2);
	float* dcw = on_device(cwt2);
	require(fi_volume_colour_constraints(raw, 1.0f, &count, dcp, dcc, dcw, FI_DEVICE) == FI_OK && same(from_device(dcp, cp.size()), cp) &&
	            same(from_device(dcc, cc.size()), cc) && same(from_device(dcw, cwt.size()), cwt),
	        "device pointers: fi_volume_colour_constraints");
	hipFree(dcp), hipFree(dcc), hipFree(dcw);
	fi_volume_destroy(raw);
	fi_volume_destroy(raw2);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, tsdf);
	put(out, weight);
	put(out, col);
	put(out, cw);
	put(out, sc);
	put(out, sv);
	put(out, depth);
	put(out, image);
	put(out, cp);
	put(out, cc);
	put(out, cwt);
	std::fclose(out);
	std::printf("all colour checks passed\n");
	return 0;
}
