// GpuLatticeField::nearest / distance_field on the points of a 3-D SDF, and the device-resident paths of the C ABI beside them.
//   test_nearest <points.bin> <out.bin>
// points.bin: int32 n, then n positions and n normals (3 floats each, lattice units), for a 40 x 36 x 32 lattice.
// The program queries the data points, a few points outside the lattice and a NaN, builds the distance field, and checks
// that fi_nearest on the context and fi_points_* with every buffer on the device (hipMalloc) give the same results bit for
// bit as the host path.  out.bin: query distances, query indices, field distances, field indices (int64 counts in front).
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
	require(argc == 3, "usage: test_nearest <points.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open points");
	int n = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "read point count");
	std::vector<float> pos(3 * n), nrm(3 * n);
	require(std::fread(pos.data(), sizeof(float), pos.size(), in) == pos.size() &&
	            std::fread(nrm.data(), sizeof(float), nrm.size(), in) == nrm.size(),
	        "read points");
	std::fclose(in);
	std::vector<float> q = pos;
	const float extra[9] = {-30.0f, 1.0f, 1.0f, 1.0f, 300.0f, 1.0f, 1.0f, 1.0f, NAN};
	q.insert(q.end(), extra, extra + 9);
	const size_t m = q.size() / 3;

	const std::vector<int> sizes = {40, 36, 32};
	std::unique_ptr<fi::GpuLatticeField> field =
	    fi::gpu_sdf_from_points(sizes, fi::Weights(), n, pos.data(), nrm.data(), nullptr);
	require(field->add_border_prior(0.001f), "add_border_prior");
	std::vector<float>     d0;
	std::vector<long long> i0;
	require(field->nearest(q, &d0, &i0) && d0.size() == m && i0.size() == m, "GpuLatticeField::nearest");
	require(std::isnan(d0[m - 1]) && i0[m - 1] == -1, "a NaN query gets NaN / -1");
	std::vector<float> d_only;
	require(field->nearest(q, &d_only) && same_bits(d_only, d0), "without indices");
	std::vector<float> near;
	std::vector<long long> near_i;
	require(field->nearest(q, &near, &near_i, 0.5f), "max_distance");
	require(std::isinf(near[m - 3]) && near_i[m - 3] == -1, "beyond max_distance: +inf / -1");
	std::vector<float>     f0;
	std::vector<long long> fi0;
	require(field->distance_field(&f0, &fi0) && f0.size() == field->num_unknowns(), "GpuLatticeField::distance_field");

	// the same through the C ABI with every buffer on the device
	float*     dq = device_buffer<float>(q.size(), q.data());
	float*     dp = device_buffer<float>(pos.size(), pos.data());
	float*     dd = device_buffer<float>(f0.size());
	long long* di = device_buffer<long long>(f0.size());
	fi_points* h  = nullptr;
	require(fi_points_create(&h, 3, n, dp, FI_DEVICE) == FI_OK, "fi_points_create, device positions");
	require(fi_points_nearest(h, static_cast<long>(m), dq, INFINITY, dd, di, FI_DEVICE) == FI_OK, "fi_points_nearest, device buffers");
	require(same_bits(from_device(dd, m), d0) && same_bits(from_device(di, m), i0), "point set = context");
	require(fi_points_distance_field(h, sizes.data(), INFINITY, dd, di, FI_DEVICE) == FI_OK, "fi_points_distance_field, device buffers");
	require(same_bits(from_device(dd, f0.size()), f0) && same_bits(from_device(di, f0.size()), fi0), "point set field = context field");
	require(fi_points_destroy(h) == FI_OK, "fi_points_destroy");
	fi_ctx* c = nullptr;
	require(fi_ctx_create(&c, 3, sizes.data(), FI_F32) == FI_OK, "fi_ctx_create");
	require(fi_add_points(c, n, dp, nullptr, nullptr, nullptr, 1.0f, FI_VALUE_LINEAR_INTERPOLATION, 0.0f, FI_GRADIENT_CELL_EDGES,
	                      FI_DEVICE) == FI_OK,
	        "fi_add_points, device positions");
	require(fi_nearest(c, static_cast<long>(m), dq, INFINITY, dd, nullptr, FI_DEVICE) == FI_OK, "fi_nearest, device buffers");
	require(same_bits(from_device(dd, m), d0), "context, device buffers = host");
	require(fi_distance_field(c, INFINITY, dd, di, FI_DEVICE) == FI_OK, "fi_distance_field, device buffers");
	require(same_bits(from_device(dd, f0.size()), f0) && same_bits(from_device(di, f0.size()), fi0), "context field, device = host");
	fi_ctx_destroy(c);
	hipFree(dq);
	hipFree(dp);
	hipFree(dd);
	hipFree(di);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, d0);
	put(out, i0);
	put(out, f0);
	put(out, fi0);
	std::fclose(out);
	std::printf("all nearest checks passed\n");
	return 0;
}
