// The plane segmentation of the C++ drop-in against the C ABI.
//   test_plane <points.bin> <out.bin>   points.bin: int32 n, then n positions (3 floats each).  segment_plane and
//                                       segment_planes are called on them and held to the bytes of fi_plane_fit and
//                                       fi_planes_segment, with host and with device pointers.
//                                       out.bin: the model as bytes, the inlier bytes, the labels, the models of
//                                       segment_planes as bytes; int64 counts in front
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
static void put(std::FILE* f, const T* p, size_t count)
{
	const long long n = static_cast<long long>(count);
	std::fwrite(&n, sizeof(n), 1, f);
	if (n) { std::fwrite(p, sizeof(T), count, f); }
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
	require(argc == 3, "usage: test_plane <points.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open points");
	int n = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "read point count");
	std::vector<float> pos(3 * n);
	require(std::fread(pos.data(), sizeof(float), pos.size(), in) == pos.size(), "read points");
	std::fclose(in);
	static_assert(sizeof(fi::PlaneModel) == sizeof(fi_plane_model), "PlaneModel mirrors fi_plane_model");

	// one plane
	fi::PlaneModel             model{};
	std::vector<unsigned char> inliers, i2(n);
	require(fi::segment_plane(3, pos, 0.15f, &model, &inliers) && static_cast<int>(inliers.size()) == n, "segment_plane");
	fi_plane_options opt{};
	opt.threshold  = 0.15f;
	opt.max_trials = 1024;
	opt.confidence = 0.999;
	opt.refine     = 2;
	fi_plane_model m2{};
	require(fi_plane_fit(3, n, pos.data(), nullptr, &opt, &m2, i2.data(), FI_HOST) == FI_OK && same(inliers, i2) &&
	            std::memcmp(&model, &m2, sizeof(m2)) == 0,
	        "... = fi_plane_fit");
	long counted = 0;
	for (unsigned char b : inliers) { counted += b; }
	require(model.found == 1 && model.inliers == counted && model.candidates == n && model.trials == 1024 && model.refits == 2,
	        "... found, and the mask holds what the model counts");
	require(model.normal[2] > 0.99 && model.rms > 0.0 && model.rms < 0.15, "... the floor");
	fi::PlaneModel alone{};
	require(fi::segment_plane(3, pos, 0.15f, &alone) && std::memcmp(&alone, &model, sizeof(model)) == 0, "... the model alone");
	std::vector<unsigned char> mask(n, 1);
	for (int i = 0; i < n; i += 3) { mask[i] = 0; }
	fi::PlaneModel masked{};
	opt.seed = 5;
	require(fi::segment_plane(3, pos, 0.15f, &masked, &inliers, 1024, 0.999, 2, 5, mask) &&
	            fi_plane_fit(3, n, pos.data(), mask.data(), &opt, &m2, i2.data(), FI_HOST) == FI_OK && same(inliers, i2) &&
	            std::memcmp(&masked, &m2, sizeof(m2)) == 0 && masked.candidates == n - (n + 2) / 3,
	        "a mask and a seed");
	fi::PlaneModel held{};
	opt.seed    = 0;
	opt.axis[0] = 1.0f;
	opt.min_cos = 0.9f;
	require(fi::segment_plane(3, pos, 0.15f, &held, nullptr, 1024, 0.999, 2, 0, {}, {1.0f, 0.0f, 0.0f}, 0.9f) &&
	            fi_plane_fit(3, n, pos.data(), nullptr, &opt, &m2, nullptr, FI_HOST) == FI_OK && std::memcmp(&held, &m2, sizeof(m2)) == 0 &&
	            held.found == 1 && std::fabs(held.normal[0]) >= 0.9 && held.inliers < model.inliers,
	        "an axis: the floor is refused");
	opt.axis[0] = 0.0f;
	opt.min_cos = 0.0f;
	require(!fi::segment_plane(3, pos, -1.0f, &model) && !fi::segment_plane(3, pos, NAN, &model) &&
	            !fi::segment_plane(3, pos, std::numeric_limits<float>::infinity(), &model) && !fi::segment_plane(1, pos, 0.1f, &model) &&
	            !fi::segment_plane(3, pos, 0.1f, nullptr) && !fi::segment_plane(3, pos, 0.1f, &model, nullptr, 0) &&
	            !fi::segment_plane(3, pos, 0.1f, &model, nullptr, 1024, 1.0) && !fi::segment_plane(3, pos, 0.1f, &model, nullptr, 1024, 0.9, 17),
	        "... a bad threshold, one dimension, a null model, no trials, confidence 1, seventeen refits are refused");
	require(fi::segment_plane(3, pos, 0.15f, &model, &inliers), "segment_plane again");

	// the same call with device pointers
	float*         dp = on_device(pos);
	unsigned char* di = on_device(i2);
	require(fi_plane_fit(3, n, dp, nullptr, &opt, &m2, di, FI_DEVICE) == FI_OK && same(from_device(di, n), inliers) &&
	            std::memcmp(&model, &m2, sizeof(m2)) == 0,
	        "device pointers: the model and the inliers");

	// several planes
	std::vector<int>            labels, l2(n);
	std::vector<fi::PlaneModel> models;
	std::vector<fi_plane_model> rows(3);
	int                         found = -1;
	require(fi::segment_planes(3, pos, 0.15f, 3, &labels, &models, 400) && static_cast<int>(labels.size()) == n, "segment_planes");
	require(fi_planes_segment(3, n, pos.data(), nullptr, &opt, 3, 400, l2.data(), rows.data(), &found, FI_HOST) == FI_OK && same(labels, l2) &&
	            found == static_cast<int>(models.size()) && std::memcmp(models.data(), rows.data(), sizeof(fi_plane_model) * found) == 0,
	        "... = fi_planes_segment");
	require(found == 1 && std::memcmp(&models[0], &model, sizeof(model)) == 0, "... the first plane is segment_plane's, and the only one of 400");
	long labelled = 0, apart = 0;
	for (int i = 0; i < n; ++i) {
		labelled += labels[i] == 0;
		apart += labels[i] != (inliers[i] ? 0 : -1);
	}
	require(labelled == model.inliers && apart == 0, "... the labels follow the inliers");
	int* dl = on_device(l2);
	require(fi_planes_segment(3, n, dp, nullptr, &opt, 3, 400, dl, rows.data(), &found, FI_DEVICE) == FI_OK && same(from_device(dl, n), labels) &&
	            found == 1 && std::memcmp(models.data(), rows.data(), sizeof(fi_plane_model)) == 0,
	        "device pointers: labels and models");
	require(!fi::segment_planes(3, pos, 0.15f, 0, &labels, &models) && !fi::segment_planes(3, pos, 0.15f, 2, nullptr, &models) &&
	            !fi::segment_planes(3, pos, 0.15f, 2, &labels, &models, -1),
	        "... no planes, a null output, a negative min_inliers are refused");
	require(fi::segment_planes(3, pos, 0.15f, 3, &labels, &models, 400), "segment_planes again");
	hipFree(dl), hipFree(di), hipFree(dp);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, reinterpret_cast<const unsigned char*>(&model), sizeof(model));
	put(out, inliers.data(), inliers.size());
	put(out, labels.data(), labels.size());
	put(out, reinterpret_cast<const unsigned char*>(models.data()), models.size() * sizeof(fi::PlaneModel));
	std::fclose(out);
	std::printf("all plane checks passed\n");
	return 0;
}
