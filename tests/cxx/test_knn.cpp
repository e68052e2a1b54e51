// GpuLatticeField::knn / estimate_normals on the points of a 3-D SDF, and the device-resident paths of the C ABI beside them.
//   test_knn <points.bin> <out.bin>
// points.bin: int32 n, then n positions (3 floats each, lattice units), for a 40 x 36 x 32 lattice.
// The program queries the data points, a point outside the lattice and a NaN for their 10 nearest points, estimates the
// normals of the data points towards one viewpoint, and checks that fi_knn / fi_estimate_normals on a context and
// fi_points_* with every buffer on the device (hipMalloc) give the same results bit for bit as the host path.
// out.bin: knn distances, knn indices, normals, variation (int64 counts in front).
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
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b)
{
	return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

template <typename T>
static void put(std::FILE* f, const std::vector<T>& v)
{
	const long long n = static_cast<long long>(v.size());
	std::fwrite(&n, sizeof(n), 1, f);
	if (n) { std::fwrite(v.data(), sizeof(T), v.size(), f); }
}

template <typename T>
static T* device_buffer(size_t n, const T* init = nullptr)
{
	void* p = nullptr;
	require(hipMalloc(&p, n * sizeof(T) + 16) == hipSuccess, "hipMalloc");
	if (init) { require(hipMemcpy(p, init, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess, "upload"); }
	return static_cast<T*>(p);
}

template <typename T>
static std::vector<T> from_device(const T* p, size_t n)
{
	std::vector<T> h(n);
	require(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess, "download");
	return h;
}

int main(int argc, char** argv)
{
	require(argc == 3, "usage: test_knn <points.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open points");
	int n = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "read point count");
	std::vector<float> pos(3 * n);
	require(std::fread(pos.data(), sizeof(float), pos.size(), in) == pos.size(), "read points");
	std::fclose(in);
	std::vector<float> q = pos;
	const float extra[6] = {-30.0f, 1.0f, 1.0f, 1.0f, 1.0f, NAN};
	q.insert(q.end(), extra, extra + 6);
	const size_t m = q.size() / 3;
	const int    k = 10;

	const std::vector<int> sizes = {40, 36, 32};
	std::unique_ptr<fi::GpuLatticeField> field = fi::gpu_sdf_from_points(sizes, fi::Weights(), n, pos.data(), nullptr, nullptr);
	require(field->add_border_prior(0.001f), "add_border_prior");
	std::vector<float>     d0;
	std::vector<long long> i0;
	require(field->knn(q, k, &d0, &i0) && d0.size() == m * k && i0.size() == m * k, "GpuLatticeField::knn");
	require(std::isnan(d0[m * k - 1]) && i0[m * k - 1] == -1, "a NaN query gets NaN / -1");
	require(d0[0] == 0.0f, "a data point finds itself");
	std::vector<float> d_only;
	require(field->knn(q, k, &d_only) && same_bits(d_only, d0), "without indices");
	require(!field->knn(q, 33, &d_only), "k = 33 is refused");
	std::vector<float>     near;
	std::vector<long long> near_i;
	require(field->knn(q, k, &near, &near_i, 0.5f), "max_distance");
	require(std::isinf(near[(m - 2) * k]) && near_i[(m - 2) * k] == -1, "beyond max_distance: +inf / -1");
	const std::vector<float> view = {-40.0f, 17.5f, 15.5f};
	std::vector<float>       n0, v0, n_plain;
	require(field->estimate_normals(&n0, 12, view, &v0) && n0.size() == pos.size() && v0.size() == static_cast<size_t>(n),
	        "GpuLatticeField::estimate_normals");
	require(field->estimate_normals(&n_plain) && n_plain.size() == pos.size(), "defaults: k = 16, the canonical sign");
	require(!field->estimate_normals(&n_plain, 2), "k = 2 < 3 is refused");

	// the same through the C ABI with every buffer on the device
	float*     dq = device_buffer<float>(q.size(), q.data());
	float*     dp = device_buffer<float>(pos.size(), pos.data());
	float*     dv = device_buffer<float>(view.size(), view.data());
	float*     dd = device_buffer<float>(m * k);
	long long* di = device_buffer<long long>(m * k);
	float*     dn = device_buffer<float>(pos.size());
	float*     dvar = device_buffer<float>(n);
	fi_points* h  = nullptr;
	require(fi_points_create(&h, 3, n, dp, FI_DEVICE) == FI_OK, "fi_points_create, device positions");
	require(fi_points_knn(h, static_cast<long>(m), dq, k, INFINITY, dd, di, FI_DEVICE) == FI_OK, "fi_points_knn, device buffers");
	require(same_bits(from_device(dd, m * k), d0) && same_bits(from_device(di, m * k), i0), "point set = context");
	require(fi_points_estimate_normals(h, 12, INFINITY, FI_ORIENT_VIEWPOINTS, dv, 1, dn, dvar, FI_DEVICE) == FI_OK,
	        "fi_points_estimate_normals, device buffers");
	require(same_bits(from_device(dn, pos.size()), n0) && same_bits(from_device(dvar, n), v0), "point set normals = context");
	require(fi_points_destroy(h) == FI_OK, "fi_points_destroy");
	fi_ctx* c = nullptr;
	require(fi_ctx_create(&c, 3, sizes.data(), FI_F32) == FI_OK, "fi_ctx_create");
	require(fi_add_points(c, n, dp, nullptr, nullptr, nullptr, 1.0f, FI_VALUE_LINEAR_INTERPOLATION, 0.0f, FI_GRADIENT_CELL_EDGES,
	                      FI_DEVICE) == FI_OK,
	        "fi_add_points, device positions");
	require(fi_knn(c, static_cast<long>(m), dq, k, INFINITY, dd, nullptr, FI_DEVICE) == FI_OK, "fi_knn, device buffers");
	require(same_bits(from_device(dd, m * k), d0), "context, device buffers = host");
	require(fi_estimate_normals(c, 12, INFINITY, FI_ORIENT_VIEWPOINTS, dv, 1, dn, nullptr, FI_DEVICE) == FI_OK,
	        "fi_estimate_normals, device buffers");
	require(same_bits(from_device(dn, pos.size()), n0), "context normals, device = host");
	fi_ctx_destroy(c);
	hipFree(dq);
	hipFree(dp);
	hipFree(dv);
	hipFree(dd);
	hipFree(di);
	hipFree(dn);
	hipFree(dvar);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, d0);
	put(out, i0);
	put(out, n0);
	put(out, v0);
	std::fclose(out);
	std::printf("all knn checks passed\n");
	return 0;
}
