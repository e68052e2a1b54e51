// The march calls of the C++ drop-in against the C ABI.
//   test_march <case.bin> <out.bin>   case.bin: int32 sizes[3], the tsdf and the weight of a volume over them, one camera (12
//                                     pose floats, fx, fy, cx, cy, int32 width, height, range (1 / 0)), int32 n, n origins and
//                                     n directions (3 floats each).  DepthVolume::raycast / render and
//                                     GpuLatticeField::march / render are called on them and held to the C ABI's bytes, with
//                                     host and with device pointers.
//                                     out.bin: t, positions, normals, side of the rays; depth, positions, normals, incidence
//                                     of the image; int64 counts in front
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
	require(argc == 3, "usage: test_march <case.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open the case");
	std::vector<int> sizes(3);
	require(std::fread(sizes.data(), sizeof(int), 3, in) == 3, "read the sizes");
	const size_t       nvox = static_cast<size_t>(sizes[0]) * sizes[1] * sizes[2];
	std::vector<float> tsdf(nvox), weight(nvox);
	require(std::fread(tsdf.data(), sizeof(float), nvox, in) == nvox && std::fread(weight.data(), sizeof(float), nvox, in) == nvox, "read the volume");
	fi::DepthCamera cam;
	int             range = 0, n = 0;
	require(std::fread(cam.pose, sizeof(float), 12, in) == 12 && std::fread(&cam.fx, sizeof(float), 1, in) == 1 &&
	            std::fread(&cam.fy, sizeof(float), 1, in) == 1 && std::fread(&cam.cx, sizeof(float), 1, in) == 1 &&
	            std::fread(&cam.cy, sizeof(float), 1, in) == 1 && std::fread(&cam.width, sizeof(int), 1, in) == 1 &&
	            std::fread(&cam.height, sizeof(int), 1, in) == 1 && std::fread(&range, sizeof(int), 1, in) == 1,
	        "read the camera");
	cam.range = range != 0;
	fi_camera ccam{};
	std::memcpy(ccam.pose, cam.pose, sizeof(cam.pose));
	ccam.fx = cam.fx, ccam.fy = cam.fy, ccam.cx = cam.cx, ccam.cy = cam.cy;
	ccam.width = cam.width, ccam.height = cam.height, ccam.kind = cam.range ? FI_DEPTH_RANGE : FI_DEPTH_Z;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "read the ray count");
	std::vector<float> o(3 * static_cast<size_t>(n)), d(o.size());
	require(std::fread(o.data(), sizeof(float), o.size(), in) == o.size() && std::fread(d.data(), sizeof(float), d.size(), in) == d.size(),
	        "read the rays");
	std::fclose(in);
	const size_t N = static_cast<size_t>(n), P = static_cast<size_t>(cam.width) * cam.height;
	const float  inf = std::numeric_limits<float>::infinity();

	fi_march_options copt{};
	require(fi_march_default_options(&copt) == FI_OK && copt.iso == 0.0f && copt.step == 1.0f && copt.min_weight == 0.0f && copt.refine == 4 &&
	            copt.side == FI_MARCH_FRONT,
	        "fi_march_default_options");
	fi::MarchOptions opt;
	opt.step = copt.step = 0.7f;
	opt.side  = fi::MarchSide::kEither;
	copt.side = FI_MARCH_EITHER;

	// rays against the volume
	fi::DepthVolume volume(sizes, 3.0f);
	require(volume.valid() && volume.load(tsdf, weight), "DepthVolume");
	std::vector<float>       t, pos, nrm, t2(N), pos2(3 * N), nrm2(3 * N);
	std::vector<signed char> side, side2(N);
	require(volume.raycast(o, d, &t, opt, &pos, &nrm, &side) && t.size() == N && pos.size() == 3 * N && side.size() == N, "DepthVolume::raycast");
	require(fi_volume_raycast(volume.handle(), &copt, n, o.data(), d.data(), 0.0f, inf, t2.data(), pos2.data(), nrm2.data(), side2.data(), FI_HOST) ==
	                FI_OK &&
	            same(t, t2) && same(pos, pos2) && same(nrm, nrm2) && same(side, side2),
	        "... = fi_volume_raycast");
	long hits = 0;
	for (signed char s : side) { hits += s != 0; }
	require(hits > n / 10, "... the rays reach the surface");
	std::vector<float> only;
	require(volume.raycast(o, d, &only, opt) && same(only, t), "... t alone");
	float *      dor = on_device(o), *ddr = on_device(d), *dt = on_device(t2), *dp = on_device(pos2), *dn = on_device(nrm2);
	signed char* ds = on_device(side2);
	require(fi_volume_raycast(volume.handle(), &copt, n, dor, ddr, 0.0f, inf, dt, dp, dn, ds, FI_DEVICE) == FI_OK && same(from_device(dt, N), t) &&
	            same(from_device(dp, 3 * N), pos) && same(from_device(dn, 3 * N), nrm) && same(from_device(ds, N), side),
	        "device pointers: fi_volume_raycast");
	float *df = on_device(tsdf), *dw = on_device(weight);
	require(fi_field_raycast(df, dw, 3, sizes.data(), &copt, n, dor, ddr, 0.0f, inf, dt, nullptr, nullptr, ds, FI_DEVICE) == FI_OK &&
	            same(from_device(dt, N), t) && same(from_device(ds, N), side),
	        "device pointers: fi_field_raycast of the same arrays");
	require(fi_field_raycast(tsdf.data(), weight.data(), 3, sizes.data(), &copt, n, o.data(), d.data(), 0.0f, inf, t2.data(), nullptr, nullptr, nullptr,
	                         FI_HOST) == FI_OK &&
	            same(t2, t),
	        "fi_field_raycast, host");
	fi::MarchOptions bad = opt;
	bad.step             = 0.0f;
	require(!volume.raycast(o, d, nullptr) && !volume.raycast(o, std::vector<float>(3), &only) && !volume.raycast(o, d, &only, bad),
	        "... no output, unpaired rays, a zero step are refused");

	// an image of the volume
	std::vector<float> depth, ip, inr, inc, depth2(P), ip2(3 * P), inr2(3 * P), inc2(P);
	require(volume.render(cam, &depth, opt, &ip, &inr, &inc) && depth.size() == P && ip.size() == 3 * P && inc.size() == P, "DepthVolume::render");
	require(fi_volume_render(volume.handle(), &copt, &ccam, depth2.data(), ip2.data(), inr2.data(), inc2.data(), FI_HOST) == FI_OK &&
	            same(depth, depth2) && same(ip, ip2) && same(inr, inr2) && same(inc, inc2),
	        "... = fi_volume_render");
	long seen = 0;
	for (float z : depth) { seen += z < inf; }
	require(seen > static_cast<long>(P) / 20, "... the image shows the surface");
	require(volume.render(cam, &only, opt) && same(only, depth), "... the depth alone");
	float *dd = on_device(depth2), *dip = on_device(ip2), *dinr = on_device(inr2), *dinc = on_device(inc2);
	require(fi_volume_render(volume.handle(), &copt, &ccam, dd, dip, dinr, dinc, FI_DEVICE) == FI_OK && same(from_device(dd, P), depth) &&
	            same(from_device(dip, 3 * P), ip) && same(from_device(dinr, 3 * P), inr) && same(from_device(dinc, P), inc),
	        "device pointers: fi_volume_render");
	require(fi_field_render(df, dw, sizes.data(), &copt, &ccam, dd, nullptr, nullptr, dinc, FI_DEVICE) == FI_OK && same(from_device(dd, P), depth) &&
	            same(from_device(dinc, P), inc),
	        "device pointers: fi_field_render of the same arrays");
	fi::DepthCamera empty = cam;
	empty.width           = 0;
	require(!volume.render(cam, nullptr) && !volume.render(empty, &only), "... no output and an empty image are refused");
	// the image goes back into a volume as it is
	fi::DepthVolume again(sizes, 3.0f);
	require(again.integrate(std::vector<fi::DepthCamera>{cam}, depth, inc), "... integrate takes the image and its incidences");

	// a solved field: the band of the volume as data, marched without a mesh
	fi::GpuLatticeField field(sizes);
	field.add_field_constraints(fi::Weights());
	std::vector<float> none;
	require(!field.march(o, d, &none, opt) && !field.render(cam, &none, opt), "march and render before a solve are refused");
	require(field.add_volume(volume, 1.0f), "add_volume");
	const std::vector<float> x = field.solve_with_guess(std::vector<float>(nvox, 0.0f), 60, 1e-3f);
	require(x.size() == nvox, "solve");
	std::vector<float>       ft, fpos, fnrm;
	std::vector<signed char> fside;
	require(field.march(o, d, &ft, opt, &fpos, &fnrm, &fside) && ft.size() == N, "GpuLatticeField::march");
	require(fi_field_raycast(x.data(), nullptr, 3, sizes.data(), &copt, n, o.data(), d.data(), 0.0f, inf, t2.data(), pos2.data(), nrm2.data(),
	                         side2.data(), FI_HOST) == FI_OK &&
	            same(ft, t2) && same(fpos, pos2) && same(fnrm, nrm2) && same(fside, side2),
	        "... = fi_field_raycast of the solution");
	std::vector<float> fdepth, fip, finr, finc;
	require(field.render(cam, &fdepth, opt, &fip, &finr, &finc) && fdepth.size() == P, "GpuLatticeField::render");
	require(fi_field_render(x.data(), nullptr, sizes.data(), &copt, &ccam, depth2.data(), ip2.data(), inr2.data(), inc2.data(), FI_HOST) == FI_OK &&
	            same(fdepth, depth2) && same(fip, ip2) && same(finr, inr2) && same(finc, inc2),
	        "... = fi_field_render of the solution");
	hipFree(dor), hipFree(ddr), hipFree(dt), hipFree(dp), hipFree(dn), hipFree(ds), hipFree(df), hipFree(dw);
	hipFree(dd), hipFree(dip), hipFree(dinr), hipFree(dinc);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, t);
	put(out, pos);
	put(out, nrm);
	put(out, side);
	put(out, depth);
	put(out, ip);
	put(out, inr);
	put(out, inc);
	std::fclose(out);
	std::printf("all march checks passed\n");
	return 0;
}
