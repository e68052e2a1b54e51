// GpuLatticeField::orient_normals on the points of a 3-D SDF, and the device-resident paths of the C ABI beside it.
//   test_orient <points.bin> <out.bin>
// points.bin: int32 n, then n positions and n normals (3 floats each), for a 40 x 36 x 32 lattice.
// The program orients the normals without a guide and with one viewpoint as a vote, and checks that fi_orient_normals on a
// context and fi_points_orient_normals with every buffer on the device (hipMalloc) give the same results bit for bit as the
// host path.  out.bin: the normals and components without a guide, then with the viewpoint (int64 counts in front).
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
	require(argc == 3, "usage: test_orient <points.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open points");
	int n = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "read point count");
	std::vector<float> pos(3 * n), nrm(3 * n);
	require(std::fread(pos.data(), sizeof(float), pos.size(), in) == pos.size(), "read points");
	require(std::fread(nrm.data(), sizeof(float), nrm.size(), in) == nrm.size(), "read normals");
	std::fclose(in);
	const int k = 10;

	const std::vector<int> sizes = {40, 36, 32};
	std::unique_ptr<fi::GpuLatticeField> field = fi::gpu_sdf_from_points(sizes, fi::Weights(), n, pos.data(), nullptr, nullptr);
	require(field->add_border_prior(0.001f), "add_border_prior");
	const std::vector<float> view = {-400.0f, 17.5f, 15.5f};
	std::vector<float>       n0 = nrm, n1 = nrm, n2 = nrm, shorter(nrm.begin(), nrm.end() - 3);
	std::vector<long long>   c0, c1;
	require(field->orient_normals(&n0, k, std::vector<float>(), &c0) && n0.size() == nrm.size() && c0.size() == static_cast<size_t>(n),
	        "GpuLatticeField::orient_normals");
	require(field->orient_normals(&n1, k, view, &c1) && same_bits(c0, c1), "with a viewpoint: the same components");
	require(field->orient_normals(&n2, k) && same_bits(n2, n0), "without components");
	require(!field->orient_normals(&n2, 33), "k = 33 is refused");
	require(!field->orient_normals(&shorter, k), "normals of the wrong size are refused");
	require(same_bits(n2, n0), "a refused call leaves the normals alone");

	// the same through the C ABI with every buffer on the device
	float*     dp = device_buffer<float>(pos.size(), pos.data());
	float*     dv = device_buffer<float>(view.size(), view.data());
	float*     dn = device_buffer<float>(nrm.size(), nrm.data());
	long long* dc = device_buffer<long long>(n);
	fi_points* h  = nullptr;
	require(fi_points_create(&h, 3, n, dp, FI_DEVICE) == FI_OK, "fi_points_create, device positions");
	require(fi_points_orient_normals(h, k, INFINITY, FI_ORIENT_NONE, nullptr, 0, dn, dc, FI_DEVICE) == FI_OK,
	        "fi_points_orient_normals, device buffers");
	require(same_bits(from_device(dn, nrm.size()), n0) && same_bits(from_device(dc, n), c0), "point set = context");
	require(hipMemcpy(dn, nrm.data(), nrm.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess, "upload");
	require(fi_points_orient_normals(h, k, INFINITY, FI_ORIENT_VIEWPOINTS, dv, 1, dn, nullptr, FI_DEVICE) == FI_OK,
	        "fi_points_orient_normals, a device viewpoint");
	require(same_bits(from_device(dn, nrm.size()), n1), "point set with a viewpoint = context");
	require(fi_points_orient_normals(h, k, INFINITY, FI_ORIENT_VIEWPOINTS, dv, 1, dn, nullptr, FI_DEVICE) == FI_OK &&
	            same_bits(from_device(dn, nrm.size()), n1),
	        "oriented normals stay as they are");
	require(fi_points_destroy(h) == FI_OK, "fi_points_destroy");
	fi_ctx* c = nullptr;
	require(fi_ctx_create(&c, 3, sizes.data(), FI_F32) == FI_OK, "fi_ctx_create");
	require(fi_add_points(c, n, dp, nullptr, nullptr, nullptr, 1.0f, FI_VALUE_LINEAR_INTERPOLATION, 0.0f, FI_GRADIENT_CELL_EDGES,
	                      FI_DEVICE) == FI_OK,
	        "fi_add_points, device positions");
	require(hipMemcpy(dn, nrm.data(), nrm.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess, "upload");
	require(fi_orient_normals(c, k, INFINITY, FI_ORIENT_VIEWPOINTS, dv, 1, dn, dc, FI_DEVICE) == FI_OK, "fi_orient_normals, device buffers");
	require(same_bits(from_device(dn, nrm.size()), n1) && same_bits(from_device(dc, n), c1), "context, device buffers = host");
	fi_ctx_destroy(c);
	hipFree(dp);
	hipFree(dv);
	hipFree(dn);
	hipFree(dc);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, n0);
	put(out, c0);
	put(out, n1);
	put(out, c1);
	std::fclose(out);
	std::printf("all orient checks passed\n");
	return 0;
}
