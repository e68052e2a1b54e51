// GpuLatticeField::redistance on a solved 3-D SDF, and the device-resident paths of fi_surface_* / fi_redistance_field.
//   test_surface <points.bin> <out.bin>
// points.bin: int32 n, then n positions and n normals (3 floats each, lattice units), for a 40 x 36 x 32 lattice.
// The program solves, redistances the solution with both methods, and checks that fi_redistance_field on a device copy of the
// solution, and fi_surface_distance_field on surfaces made from the returned mesh (fi_surface_from_mesh), from its arrays
// on the host and from its arrays on the device, give the same results bit for bit.  It then queries 2000 off-lattice
// points and a NaN against the three surfaces.  out.bin (int64 counts in front of each): the solution, the iso method's
// distances and primitives, the dual method's distances and primitives, the mesh's vertices and indices, the queries and
// their distances, primitives and closest points.
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
	require(argc == 3, "usage: test_surface <points.bin> <out.bin>");
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
	std::unique_ptr<fi::GpuLatticeField> field = fi::gpu_sdf_from_points(sizes, fi::Weights(), n, pos.data(), nrm.data(), nullptr);
	std::vector<float>     d0, d1;
	std::vector<long long> p0, p1;
	require(!field->redistance(&d0), "redistance before a solve fails");
	field->set_levels(3, true);
	const std::vector<float> x = field->solve(0, 1e-6f);
	require(x.size() == field->num_unknowns(), "solve");
	require(field->redistance(&d0, 0.0f, false, INFINITY, &p0) && d0.size() == x.size(), "GpuLatticeField::redistance, iso");
	require(field->redistance(&d1, 0.0f, true, INFINITY, &p1) && d1.size() == x.size(), "GpuLatticeField::redistance, dual");
	std::vector<float> d_only;
	require(field->redistance(&d_only) && same_bits(d_only, d0), "without primitives");

	// the same through the C ABI with every buffer on the device
	const size_t total = x.size();
	float*       dx    = device_buffer<float>(total, x.data());
	float*       dd    = device_buffer<float>(total);
	long long*   dp    = device_buffer<long long>(total);
	fi_mesh*     m     = nullptr;
	require(fi_redistance_field(dx, 3, sizes.data(), 0.0f, FI_SURFACE_ISO, INFINITY, dd, dp, &m, FI_DEVICE) == FI_OK,
	        "fi_redistance_field, device buffers");
	require(same_bits(from_device(dd, total), d0) && same_bits(from_device(dp, total), p0), "device field = solution in place");
	long nv = 0, np = 0;
	int  vpp = 0;
	require(fi_mesh_info(m, &nv, &np, &vpp) == FI_OK && vpp == 3 && np > 0, "fi_mesh_info");
	std::vector<float> v(3 * nv);
	std::vector<int>   idx(3 * np);
	require(fi_mesh_copy(m, v.data(), nullptr, idx.data(), nullptr, FI_HOST) == FI_OK, "fi_mesh_copy");

	fi_surface* s[3] = {nullptr, nullptr, nullptr};
	require(fi_surface_from_mesh(&s[0], m) == FI_OK, "fi_surface_from_mesh");
	require(fi_surface_create(&s[1], 3, nv, v.data(), np, idx.data(), FI_HOST) == FI_OK, "fi_surface_create, host arrays");
	float* dv = device_buffer<float>(v.size(), v.data());
	int*   di = device_buffer<int>(idx.size(), idx.data());
	require(fi_surface_create(&s[2], 3, nv, dv, np, di, FI_DEVICE) == FI_OK, "fi_surface_create, device arrays");
	fi_mesh_destroy(m);
	std::vector<float> absd(total);
	for (size_t k = 0; k < total; ++k) { absd[k] = std::fabs(d0[k]); }

	const size_t       nq = 2001;
	std::vector<float> q(3 * nq);
	for (size_t k = 0; k < nq; ++k) {
		for (int d = 0; d < 3; ++d) { q[3 * k + d] = std::fmod(0.6180339f * (3 * k + d) * (d + 1.37f), sizes[d] + 6.0f) - 3.0f; }
	}
	q[3 * (nq - 1) + 1] = NAN;
	float*                 dq = device_buffer<float>(q.size(), q.data());
	float*                 qd = device_buffer<float>(nq);
	long long*             qp = device_buffer<long long>(nq);
	float*                 qc = device_buffer<float>(3 * nq);
	std::vector<float>     qd0, qc0;
	std::vector<long long> qp0;
	for (int k = 0; k < 3; ++k) {
		require(fi_surface_distance_field(s[k], sizes.data(), INFINITY, dd, dp, FI_DEVICE) == FI_OK, "fi_surface_distance_field");
		require(same_bits(from_device(dd, total), absd) && same_bits(from_device(dp, total), p0), "distance field = |redistance|");
		require(fi_surface_distance(s[k], static_cast<long>(nq), dq, INFINITY, qd, qp, qc, FI_DEVICE) == FI_OK, "fi_surface_distance");
		if (k == 0) {
			qd0 = from_device(qd, nq);
			qp0 = from_device(qp, nq);
			qc0 = from_device(qc, 3 * nq);
		} else {
			require(same_bits(from_device(qd, nq), qd0) && same_bits(from_device(qp, nq), qp0) && same_bits(from_device(qc, 3 * nq), qc0),
			        "every way of making the surface gives the same queries");
		}
		require(fi_surface_destroy(s[k]) == FI_OK, "fi_surface_destroy");
	}
	require(std::isnan(qd0[nq - 1]) && qp0[nq - 1] == -1, "a NaN query gets NaN / -1");
	for (void* p : {static_cast<void*>(dx), static_cast<void*>(dd), static_cast<void*>(dp), static_cast<void*>(dv), static_cast<void*>(di),
	                static_cast<void*>(dq), static_cast<void*>(qd), static_cast<void*>(qp), static_cast<void*>(qc)}) {
		hipFree(p);
	}

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, x);
	put(out, d0);
	put(out, p0);
	put(out, d1);
	put(out, p1);
	put(out, v);
	put(out, idx);
	put(out, q);
	put(out, qd0);
	put(out, qp0);
	put(out, qc0);
	std::fclose(out);
	std::printf("all surface checks passed\n");
	return 0;
}
