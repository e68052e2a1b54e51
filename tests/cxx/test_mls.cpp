// The moving-least-squares calls of the C++ drop-in against the C ABI.
//   test_mls <points.bin> <out.bin>   points.bin: int32 n, then n positions and n guide normals (3 floats each, lattice units)
//                                     for a 32 x 32 x 32 lattice.  The points become the data points of a field (no solve is
//                                     needed); GpuLatticeField::smooth_points and the free smooth_points are called on them
//                                     and held to the C ABI's bytes on a fi_points of the same cloud, with host and with
//                                     device pointers.
//                                     out.bin: positions, normals, curvature and order of the quadric with guide normals,
//                                     then positions and order of the plane; int64 counts in front
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
	require(argc == 3, "usage: test_mls <points.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open points");
	int n = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "read point count");
	std::vector<float> pos(3 * n), guide(3 * n);
	require(std::fread(pos.data(), sizeof(float), pos.size(), in) == pos.size() &&
	            std::fread(guide.data(), sizeof(float), guide.size(), in) == guide.size(),
	        "read points");
	std::fclose(in);

	const std::vector<int> sizes = {32, 32, 32};
	std::unique_ptr<fi::GpuLatticeField> field = fi::gpu_sdf_from_points(sizes, fi::Weights(), n, pos.data(), guide.data(), nullptr);
	fi_points* set = nullptr;
	require(fi_points_create(&set, 3, n, pos.data(), FI_HOST) == FI_OK, "fi_points_create");
	const float inf = std::numeric_limits<float>::infinity();

	// the quadric, every output, guide normals, a limited move
	std::vector<float>         p, nr, cu, p2(3 * n), nr2(3 * n), cu2(n);
	std::vector<unsigned char> od, od2(n);
	require(field->smooth_points(2.5f, &p, &nr, 32, 2, 0.5f, guide, &cu, &od) && static_cast<int>(od.size()) == n, "smooth_points");
	require(fi_points_mls_project(set, n, nullptr, 32, 2.5f, 2, 0.5f, guide.data(), p2.data(), nr2.data(), cu2.data(), od2.data(), FI_HOST) ==
	                FI_OK &&
	            same(p, p2) && same(nr, nr2) && same(cu, cu2) && same(od, od2),
	        "... = fi_points_mls_project");
	long fitted = 0;
	for (unsigned char o : od) { fitted += o == 2; }
	require(fitted > n / 2 && !same(p, pos), "... most points take the quadric and move");
	std::vector<float>         fp, fn, fc;
	std::vector<unsigned char> fo;
	require(fi::smooth_points(3, pos, 2.5f, &fp, &fn, 32, 2, 0.5f, guide, &fc, &fo) && same(fp, p) && same(fn, nr) && same(fc, cu) && same(fo, od),
	        "the free smooth_points gives the same bytes");

	// the plane, positions and order alone, the defaults
	std::vector<float>         q, q2(3 * n);
	std::vector<unsigned char> qo, qo2(n);
	require(field->smooth_points(2.5f, &q, nullptr, 32, 1, inf, std::vector<float>(), nullptr, &qo), "smooth_points, the plane");
	require(fi_points_mls_project(set, n, nullptr, 32, 2.5f, 1, inf, nullptr, q2.data(), nullptr, nullptr, qo2.data(), FI_HOST) == FI_OK &&
	            same(q, q2) && same(qo, qo2) && !same(q, p),
	        "... = fi_points_mls_project");
	std::vector<float> only;
	require(field->smooth_points(2.5f, nullptr, nullptr, 32, 2, 0.5f, guide, &only) && same(only, cu), "... the curvature alone");
	require(!field->smooth_points(2.5f, nullptr) && !field->smooth_points(0.0f, &only) && !field->smooth_points(2.5f, &only, nullptr, 33) &&
	            !field->smooth_points(2.5f, &only, nullptr, 32, 3) && !field->smooth_points(2.5f, &only, nullptr, 32, 2, -1.0f) &&
	            !field->smooth_points(2.5f, &only, nullptr, 32, 2, inf, std::vector<float>(5)),
	        "... no output, a zero radius, k = 33, degree 3, a negative move, a short guide are refused");
	require(!fi::smooth_points(1, pos, 2.5f, &only) && !fi::smooth_points(3, pos, NAN, &only) && !fi::smooth_points(3, pos, 2.5f, nullptr),
	        "... one dimension, a NaN radius, no output are refused");

	// the points as queries, and device pointers
	require(fi_points_mls_project(set, n, pos.data(), 32, 2.5f, 2, 0.5f, guide.data(), p2.data(), nr2.data(), cu2.data(), od2.data(),
	                              FI_HOST) == FI_OK &&
	            same(p, p2) && same(nr, nr2) && same(cu, cu2) && same(od, od2),
	        "fi_points_mls_project with the points as queries");
	float*         dq = on_device(pos);
	float*         dg = on_device(guide);
	float*         dp = on_device(pos);
	float*         dn = on_device(pos);
	float*         dc = on_device(cu2);
	unsigned char* dord = on_device(od2);
	require(fi_points_mls_project(set, n, nullptr, 32, 2.5f, 2, 0.5f, dg, dp, dn, dc, dord, FI_DEVICE) == FI_OK && same(from_device(dp, p.size()), p) &&
	            same(from_device(dn, nr.size()), nr) && same(from_device(dc, cu.size()), cu) && same(from_device(dord, od.size()), od),
	        "device pointers: the set's own points");
	require(fi_points_mls_project(set, n, dq, 32, 2.5f, 1, inf, nullptr, dp, nullptr, nullptr, dord, FI_DEVICE) == FI_OK &&
	            same(from_device(dp, q.size()), q) && same(from_device(dord, qo.size()), qo),
	        "device pointers: the points as queries");
	hipFree(dq), hipFree(dg), hipFree(dp), hipFree(dn), hipFree(dc), hipFree(dord);
	fi_points_destroy(set);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, p.data(), p.size());
	put(out, nr.data(), nr.size());
	put(out, cu.data(), cu.size());
	put(out, od.data(), od.size());
	put(out, q.data(), q.size());
	put(out, qo.data(), qo.size());
	std::fclose(out);
	std::printf("all mls checks passed\n");
	return 0;
}
