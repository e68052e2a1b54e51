// GpuLatticeField::raycast on a solved 3-D SDF, and the device-resident paths of the ray entries of fi_surface_*.
//   test_raycast <points.bin> <out.bin>
// points.bin: int32 n, then n positions and n normals (3 floats each, lattice units), for a 40 x 36 x 32 lattice.
// The program solves, casts 2001 rays at the solution's own mesh with both methods, and checks that the C entries with every
// buffer on the device (the surface from fi_iso_extract_field on a device copy of the solution) and with every buffer on
// the host give the same results bit for bit.  out.bin (int64 counts in front of each): the solution, the rays' origins and
// directions, the iso method's t and primitives, the dual method's t and primitives, the barycentrics, the counts at limit
// 2, the containment of the origins along +x and along (0, -1, 2), the signed distances of the origins with their primitives
// and closest points, and the signed distance field with its primitives.
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
	require(argc == 3, "usage: test_raycast <points.bin> <out.bin>");
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
	const size_t           nr    = 2001;
	std::vector<float>     o(3 * nr), d(3 * nr);
	for (size_t k = 0; k < nr; ++k) {
		for (int a = 0; a < 3; ++a) {
			o[3 * k + a] = std::fmod(0.6180339f * (3 * k + a) * (a + 1.37f), sizes[a] + 6.0f) - 3.0f;
			const float aim = sizes[a] * (0.3f + 0.4f * std::fmod(0.7548777f * (3 * k + a), 1.0f));
			d[3 * k + a] = (aim - o[3 * k + a]) * 0.125f;
		}
	}
	for (size_t k = 0; k < 60; ++k) {  // lattice points along the axes: through the mesh's vertices
		for (int a = 0; a < 3; ++a) {
			o[3 * k + a] = std::floor(o[3 * k + a]);
			d[3 * k + a] = a == static_cast<int>(k % 3) ? (k % 2 ? -1.0f : 1.0f) : 0.0f;
		}
	}
	o[3 * (nr - 1) + 1] = NAN;
	d[3 * (nr - 2)] = d[3 * (nr - 2) + 1] = d[3 * (nr - 2) + 2] = 0.0f;

	std::unique_ptr<fi::GpuLatticeField> field = fi::gpu_sdf_from_points(sizes, fi::Weights(), n, pos.data(), nrm.data(), nullptr);
	std::vector<float>     t0, t1, t_only;
	std::vector<long long> p0, p1;
	require(!field->raycast(o, d, &t0), "raycast before a solve fails");
	field->set_levels(3, true);
	const std::vector<float> x = field->solve(0, 1e-6f);
	require(x.size() == field->num_unknowns(), "solve");
	require(field->raycast(o, d, &t0, 0.0f, false, INFINITY, &p0) && t0.size() == nr && p0.size() == nr, "GpuLatticeField::raycast, iso");
	require(field->raycast(o, d, &t1, 0.0f, true, INFINITY, &p1) && t1.size() == nr, "GpuLatticeField::raycast, dual");
	require(field->raycast(o, d, &t_only) && same_bits(t_only, t0), "without primitives");
	require(!field->raycast(o, std::vector<float>(3), &t_only), "origins and directions of different lengths fail");
	require(std::isnan(t0[nr - 1]) && p0[nr - 1] == -1 && std::isnan(t0[nr - 2]) && p0[nr - 2] == -1, "a NaN origin and a zero direction get NaN / -1");

	// the C entries with every buffer on the device, then on the host
	const size_t total = x.size();
	float*       dx    = device_buffer<float>(total, x.data());
	fi_mesh*     m     = nullptr;
	fi_surface*  s     = nullptr;
	require(fi_iso_extract_field(dx, 3, sizes.data(), 0.0f, FI_DEVICE, &m) == FI_OK, "fi_iso_extract_field, device field");
	require(fi_surface_from_mesh(&s, m) == FI_OK, "fi_surface_from_mesh");
	fi_mesh_destroy(m);
	float*         dor = device_buffer<float>(o.size(), o.data());
	float*         ddr = device_buffer<float>(d.size(), d.data());
	float*         dt  = device_buffer<float>(nr);
	long long*     dp  = device_buffer<long long>(nr);
	float*         db  = device_buffer<float>(2 * nr);
	int*           dc  = device_buffer<int>(nr);
	unsigned char* di  = device_buffer<unsigned char>(nr);
	float*         dcl = device_buffer<float>(3 * nr);
	float*         df  = device_buffer<float>(total);
	long long*     dfp = device_buffer<long long>(total);
	const float    dir[3] = {0.0f, -1.0f, 2.0f};

	require(fi_surface_raycast(s, nr, dor, ddr, 0.0f, INFINITY, dt, dp, db, FI_DEVICE) == FI_OK, "fi_surface_raycast, device buffers");
	require(same_bits(from_device(dt, nr), t0) && same_bits(from_device(dp, nr), p0), "device rays = GpuLatticeField::raycast");
	const std::vector<float> bary = from_device(db, 2 * nr);
	std::vector<float>       ht(nr), hb(2 * nr);
	std::vector<long long>   hp(nr);
	require(fi_surface_raycast(s, nr, o.data(), d.data(), 0.0f, INFINITY, ht.data(), hp.data(), hb.data(), FI_HOST) == FI_OK,
	        "fi_surface_raycast, host buffers");
	require(same_bits(ht, t0) && same_bits(hp, p0) && same_bits(hb, bary), "host rays = device rays");

	require(fi_surface_count_hits(s, nr, dor, ddr, 0.0f, INFINITY, 2, dc, FI_DEVICE) == FI_OK, "fi_surface_count_hits, device buffers");
	const std::vector<int> counts = from_device(dc, nr);
	std::vector<int>       hc(nr);
	require(fi_surface_count_hits(s, nr, o.data(), d.data(), 0.0f, INFINITY, 2, hc.data(), FI_HOST) == FI_OK && same_bits(hc, counts),
	        "host counts = device counts");
	bool agree = true;
	for (size_t k = 0; k < nr; ++k) { agree = agree && (counts[k] > 0) == (p0[k] >= 0); }
	require(agree, "a ray counts hits exactly when it has a closest one");

	require(fi_surface_contains(s, nr, dor, nullptr, di, FI_DEVICE) == FI_OK, "fi_surface_contains, device buffers");
	const std::vector<unsigned char> in_x = from_device(di, nr);
	require(fi_surface_contains(s, nr, dor, dir, di, FI_DEVICE) == FI_OK, "fi_surface_contains along a direction");
	const std::vector<unsigned char> in_d = from_device(di, nr);
	std::vector<unsigned char>       hi(nr);
	require(fi_surface_contains(s, nr, o.data(), dir, hi.data(), FI_HOST) == FI_OK && same_bits(hi, in_d), "host containment = device containment");

	require(fi_surface_signed_distance(s, nr, dor, 4.0f, dt, dp, dcl, FI_DEVICE) == FI_OK, "fi_surface_signed_distance, device buffers");
	const std::vector<float>     sd = from_device(dt, nr), sc = from_device(dcl, 3 * nr);
	const std::vector<long long> sp = from_device(dp, nr);
	std::vector<float>           hsd(nr), hsc(3 * nr);
	require(fi_surface_signed_distance(s, nr, o.data(), 4.0f, hsd.data(), hp.data(), hsc.data(), FI_HOST) == FI_OK && same_bits(hsd, sd) &&
	            same_bits(hp, sp) && same_bits(hsc, sc),
	        "host signed distances = device signed distances");

	require(fi_surface_signed_distance_field(s, sizes.data(), INFINITY, df, dfp, FI_DEVICE) == FI_OK, "fi_surface_signed_distance_field, device buffers");
	const std::vector<float>     sf  = from_device(df, total);
	const std::vector<long long> sfp = from_device(dfp, total);
	std::vector<float>           hsf(total);
	require(fi_surface_signed_distance_field(s, sizes.data(), INFINITY, hsf.data(), nullptr, FI_HOST) == FI_OK && same_bits(hsf, sf),
	        "host signed field = device signed field");
	require(fi_surface_destroy(s) == FI_OK, "fi_surface_destroy");
	for (void* p : {static_cast<void*>(dx), static_cast<void*>(dor), static_cast<void*>(ddr), static_cast<void*>(dt), static_cast<void*>(dp),
	                static_cast<void*>(db), static_cast<void*>(dc), static_cast<void*>(di), static_cast<void*>(dcl), static_cast<void*>(df),
	                static_cast<void*>(dfp)}) {
		hipFree(p);
	}

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, x);
	put(out, o);
	put(out, d);
	put(out, t0);
	put(out, p0);
	put(out, t1);
	put(out, p1);
	put(out, bary);
	put(out, counts);
	put(out, in_x);
	put(out, in_d);
	put(out, sd);
	put(out, sp);
	put(out, sc);
	put(out, sf);
	put(out, sfp);
	std::fclose(out);
	std::printf("all raycast checks passed\n");
	return 0;
}
