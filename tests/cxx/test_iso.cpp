// GpuLatticeField::iso_surface on a solved 3-D SDF, and the device-resident paths of the C ABI beside it.
//   test_iso <points.bin> <out.bin>
// points.bin: int32 n, then n positions and n normals (3 floats each, lattice units), for a 40 x 36 x 32 lattice.
// The program solves with the V-cycle, extracts the mesh from the solution on the device, and checks that the same
// field passed as a device pointer -- fi_iso_extract on a context, fi_iso_extract_field -- with fi_mesh_copy into device
// buffers gives the same mesh bit for bit.  out.bin: the solution, then vertices, normals and indices (int64 counts in front).
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
static std::vector<T> from_device(const void* p, size_t n)
{
	std::vector<T> h(n);
	if (n) { require(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess, "hipMemcpy"); }
	return h;
}

// a mesh made from a device field, copied out into device buffers
static void device_mesh(fi_mesh* m, std::vector<float>* v, std::vector<float>* nrm, std::vector<int>* idx)
{
	long nv = 0, np = 0;
	int  vpp = 0;
	require(fi_mesh_info(m, &nv, &np, &vpp) == FI_OK && vpp == 3, "fi_mesh_info");
	void *dv = nullptr, *dn = nullptr, *di = nullptr, *dk = nullptr;
	require(hipMalloc(&dv, 12 * (nv + 1)) == hipSuccess && hipMalloc(&dn, 12 * (nv + 1)) == hipSuccess &&
	            hipMalloc(&di, 12 * (np + 1)) == hipSuccess && hipMalloc(&dk, 8 * (nv + 1)) == hipSuccess,
	        "hipMalloc");
	require(fi_mesh_copy(m, static_cast<float*>(dv), static_cast<float*>(dn), static_cast<int*>(di), static_cast<long long*>(dk),
	                     FI_DEVICE) == FI_OK,
	        "fi_mesh_copy into device buffers");
	*v   = from_device<float>(dv, 3 * nv);
	*nrm = from_device<float>(dn, 3 * nv);
	*idx = from_device<int>(di, 3 * np);
	std::vector<long long> keys = from_device<long long>(dk, nv);
	bool ascending = true;
	for (long i = 1; i < nv; ++i) { ascending = ascending && keys[i - 1] < keys[i]; }
	require(ascending, "keys ascending");
	hipFree(dv);
	hipFree(dn);
	hipFree(di);
	hipFree(dk);
	fi_mesh_destroy(m);
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

int main(int argc, char** argv)
{
	require(argc == 3, "usage: test_iso <points.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open points");
	int n = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "read point count");
	std::vector<float> pos(3 * n), nrm(3 * n);
	require(std::fread(pos.data(), sizeof(float), pos.size(), in) == pos.size() &&
	            std::fread(nrm.data(), sizeof(float), nrm.size(), in) == nrm.size(),
	        "read points");
	std::fclose(in);

	const std::vector<int> sizes = {40, 36, 32};
	std::unique_ptr<fi::GpuLatticeField> field =
	    fi::gpu_sdf_from_points(sizes, fi::Weights(), n, pos.data(), nrm.data(), nullptr);
	std::vector<float> v0, n0;
	std::vector<int>   i0;
	require(!field->iso_surface(0.0f, &v0, &i0, &n0), "iso_surface before a solve fails");
	field->set_levels(3, true);
	const std::vector<float> x = field->solve(0, 1e-6f);
	require(x.size() == field->num_unknowns(), "solve");
	require(field->iso_surface(0.0f, &v0, &i0, &n0), "GpuLatticeField::iso_surface");
	require(!v0.empty() && i0.size() % 3 == 0 && n0.size() == v0.size(), "a non-empty triangle mesh");
	std::vector<float> v_only;
	std::vector<int>   i_only;
	require(field->iso_surface(0.0f, &v_only, &i_only) && same_bits(v_only, v0) && same_bits(i_only, i0), "without normals");

	float* dx = nullptr;
	require(hipMalloc(reinterpret_cast<void**>(&dx), x.size() * sizeof(float)) == hipSuccess, "hipMalloc field");
	require(hipMemcpy(dx, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess, "upload field");

	fi_mesh* m = nullptr;
	require(fi_iso_extract_field(dx, 3, sizes.data(), 0.0f, FI_DEVICE, &m) == FI_OK, "fi_iso_extract_field from device");
	std::vector<float> v1, n1;
	std::vector<int>   i1;
	device_mesh(m, &v1, &n1, &i1);
	require(same_bits(v1, v0) && same_bits(n1, n0) && same_bits(i1, i0), "device field = solution in place");

	fi_ctx* c = nullptr;
	require(fi_ctx_create(&c, 3, sizes.data(), FI_F32) == FI_OK, "fi_ctx_create");
	require(fi_iso_extract(c, dx, 0.0f, FI_DEVICE, &m) == FI_OK, "fi_iso_extract of a device field");
	std::vector<float> v2, n2;
	std::vector<int>   i2;
	device_mesh(m, &v2, &n2, &i2);
	require(same_bits(v2, v0) && same_bits(n2, n0) && same_bits(i2, i0), "context, device field = solution in place");
	fi_ctx_destroy(c);
	hipFree(dx);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, x);
	put(out, v0);
	put(out, n0);
	put(out, i0);
	std::fclose(out);
	std::printf("all iso checks passed\n");
	return 0;
}
