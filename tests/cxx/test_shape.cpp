// The sphere and cylinder segmentation of the C++ drop-in against the C ABI.
//   test_shape <points.bin> <out.bin>   points.bin: int32 n, then n positions and n normals (3 floats each).  segment_shape
//                                       and segment_shapes are called on them and held to the bytes of fi_shape_fit and
//                                       fi_shapes_segment, with host and with device pointers.
//                                       out.bin: the cylinder's model as bytes, its inlier bytes, the sphere's model as
//                                       bytes, the labels and the models of segment_shapes as bytes; int64 counts in front
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
	require(argc == 3, "usage: test_shape <points.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open points");
	int n = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "read point count");
	std::vector<float> pos(3 * n), nrm(3 * n);
	require(std::fread(pos.data(), sizeof(float), pos.size(), in) == pos.size(), "read points");
	require(std::fread(nrm.data(), sizeof(float), nrm.size(), in) == nrm.size(), "read normals");
	std::fclose(in);
	static_assert(sizeof(fi::ShapeModel) == sizeof(fi_shape_model), "ShapeModel mirrors fi_shape_model");
	const float inf = std::numeric_limits<float>::infinity();
	const std::vector<float> none;

	// one cylinder
	fi::ShapeModel             model{};
	std::vector<unsigned char> inliers, i2(n);
	require(fi::segment_shape(3, fi::Shape::kCylinder, pos, nrm, 0.05f, &model, &inliers, 0.1f, 2.0f) && static_cast<int>(inliers.size()) == n,
	        "segment_shape, a cylinder");
	fi_shape_options opt{};
	opt.kind       = FI_SHAPE_CYLINDER;
	opt.threshold  = 0.05f;
	opt.r_min      = 0.1f;
	opt.r_max      = 2.0f;
	opt.max_trials = 1024;
	opt.confidence = 0.999;
	opt.refine     = 2;
	fi_shape_model m2{};
	require(fi_shape_fit(3, n, pos.data(), nrm.data(), nullptr, &opt, &m2, i2.data(), FI_HOST) == FI_OK && same(inliers, i2) &&
	            std::memcmp(&model, &m2, sizeof(m2)) == 0,
	        "... = fi_shape_fit");
	long counted = 0;
	for (unsigned char b : inliers) { counted += b; }
	require(model.found == 1 && model.kind == FI_SHAPE_CYLINDER && model.inliers == counted && model.candidates == n && model.refits == 2,
	        "... found, and the mask holds what the model counts");
	require(std::fabs(model.radius - 0.5) < 0.05 && model.rms > 0.0 && model.rms < 0.05 && model.extent[0] < model.extent[1], "... the pipe");
	fi::ShapeModel alone{};
	require(fi::segment_shape(3, fi::Shape::kCylinder, pos, nrm, 0.05f, &alone, nullptr, 0.1f, 2.0f) && std::memcmp(&alone, &model, sizeof(model)) == 0,
	        "... the model alone");
	std::vector<unsigned char> mask(n, 1);
	for (int i = 0; i < n; i += 3) { mask[i] = 0; }
	fi::ShapeModel masked{};
	opt.seed       = 5;
	opt.normal_cos = 0.9f;
	require(fi::segment_shape(3, fi::Shape::kCylinder, pos, nrm, 0.05f, &masked, &inliers, 0.1f, 2.0f, 0.9f, 1024, 0.999, 2, 5, mask) &&
	            fi_shape_fit(3, n, pos.data(), nrm.data(), mask.data(), &opt, &m2, i2.data(), FI_HOST) == FI_OK && same(inliers, i2) &&
	            std::memcmp(&masked, &m2, sizeof(m2)) == 0 && masked.candidates == n - (n + 2) / 3,
	        "a mask, a seed and an angle");
	opt.seed       = 0;
	opt.normal_cos = 0.0f;

	// one sphere, without normals
	fi::ShapeModel sphere{};
	opt.kind  = FI_SHAPE_SPHERE;
	opt.r_min = 0.5f;
	opt.r_max = inf;
	require(fi::segment_shape(3, fi::Shape::kSphere, pos, none, 0.05f, &sphere, nullptr, 0.5f) &&
	            fi_shape_fit(3, n, pos.data(), nullptr, nullptr, &opt, &m2, nullptr, FI_HOST) == FI_OK && std::memcmp(&sphere, &m2, sizeof(m2)) == 0 &&
	            sphere.kind == FI_SHAPE_SPHERE && sphere.axis[0] == 0.0 && sphere.extent[1] == 0.0,
	        "segment_shape, a sphere without normals = fi_shape_fit");
	require(!fi::segment_shape(3, fi::Shape::kSphere, pos, none, -1.0f, &model) && !fi::segment_shape(3, fi::Shape::kSphere, pos, none, NAN, &model) &&
	            !fi::segment_shape(1, fi::Shape::kSphere, pos, none, 0.1f, &model) && !fi::segment_shape(3, fi::Shape::kSphere, pos, none, 0.1f, nullptr) &&
	            !fi::segment_shape(3, fi::Shape::kCylinder, pos, none, 0.1f, &model) &&
	            !fi::segment_shape(3, fi::Shape::kSphere, pos, none, 0.1f, &model, nullptr, 2.0f, 1.0f) &&
	            !fi::segment_shape(3, fi::Shape::kSphere, pos, none, 0.1f, &model, nullptr, 0.0f, inf, 0.5f) &&
	            !fi::segment_shape(3, fi::Shape::kSphere, pos, none, 0.1f, &model, nullptr, 0.0f, inf, 0.0f, 0) &&
	            !fi::segment_shape(3, static_cast<fi::Shape>(7), pos, none, 0.1f, &model),
	        "... a bad threshold, one dimension, a null model, a cylinder without normals, limits the wrong way round, an angle "
	        "without normals, no trials, an unknown kind are refused");
	opt.kind  = FI_SHAPE_CYLINDER;
	opt.r_min = 0.1f;
	opt.r_max = 2.0f;
	require(fi::segment_shape(3, fi::Shape::kCylinder, pos, nrm, 0.05f, &model, &inliers, 0.1f, 2.0f), "segment_shape again");

	// the same call with device pointers
	float*         dp = on_device(pos);
	float*         dn = on_device(nrm);
	unsigned char* di = on_device(i2);
	require(fi_shape_fit(3, n, dp, dn, nullptr, &opt, &m2, di, FI_DEVICE) == FI_OK && same(from_device(di, n), inliers) &&
	            std::memcmp(&model, &m2, sizeof(m2)) == 0,
	        "device pointers: the model and the inliers");

	// several shapes
	std::vector<int>            labels, l2(n);
	std::vector<fi::ShapeModel> models;
	std::vector<fi_shape_model> rows(3);
	int                         found = -1;
	require(fi::segment_shapes(3, fi::Shape::kCylinder, pos, nrm, 0.05f, 3, &labels, &models, 400, 0.1f, 2.0f) && static_cast<int>(labels.size()) == n,
	        "segment_shapes");
	require(fi_shapes_segment(3, n, pos.data(), nrm.data(), nullptr, &opt, 3, 400, l2.data(), rows.data(), &found, FI_HOST) == FI_OK &&
	            same(labels, l2) && found == static_cast<int>(models.size()) &&
	            std::memcmp(models.data(), rows.data(), sizeof(fi_shape_model) * found) == 0,
	        "... = fi_shapes_segment");
	require(found >= 1 && std::memcmp(&models[0], &model, sizeof(model)) == 0, "... the first shape is segment_shape's");
	long labelled = 0, apart = 0;
	for (int i = 0; i < n; ++i) {
		labelled += labels[i] == 0;
		apart += (labels[i] == 0) != (inliers[i] != 0);
	}
	require(labelled == model.inliers && apart == 0, "... the labels follow the inliers");
	int* dl = on_device(l2);
	const int host_found = found;
	require(fi_shapes_segment(3, n, dp, dn, nullptr, &opt, 3, 400, dl, rows.data(), &found, FI_DEVICE) == FI_OK && same(from_device(dl, n), labels) &&
	            found == host_found && std::memcmp(models.data(), rows.data(), sizeof(fi_shape_model) * found) == 0,
	        "device pointers: labels and models");
	require(!fi::segment_shapes(3, fi::Shape::kCylinder, pos, nrm, 0.05f, 0, &labels, &models) &&
	            !fi::segment_shapes(3, fi::Shape::kCylinder, pos, nrm, 0.05f, 2, nullptr, &models) &&
	            !fi::segment_shapes(3, fi::Shape::kCylinder, pos, nrm, 0.05f, 2, &labels, &models, -1),
	        "... no shapes, a null output, a negative min_inliers are refused");
	require(fi::segment_shapes(3, fi::Shape::kCylinder, pos, nrm, 0.05f, 3, &labels, &models, 400, 0.1f, 2.0f), "segment_shapes again");
	hipFree(dl), hipFree(di), hipFree(dn), hipFree(dp);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, reinterpret_cast<const unsigned char*>(&model), sizeof(model));
	put(out, inliers.data(), inliers.size());
	put(out, reinterpret_cast<const unsigned char*>(&sphere), sizeof(sphere));
	put(out, labels.data(), labels.size());
	put(out, reinterpret_cast<const unsigned char*>(models.data()), models.size() * sizeof(fi::ShapeModel));
	std::fclose(out);
	std::printf("all shape checks passed\n");
	return 0;
}
