// GpuLatticeField::iso_surface_points on a solved 3-D SDF.
//   test_meshpts <points.bin> <out.bin>   points.bin: int32 n, then n positions and n normals (3 floats each, lattice units) for a
//                                         40 x 36 x 32 lattice; solves with the V-cycle, spreads oriented points over the
//                                         iso-surface of the solution with both extractors, and walks the C ABI (fi_mesh_sample,
//                                         fi_mesh_deviation with device pointers) against it.
//                                         out.bin: the solution, then the positions and normals of the 5000 points of seed 9 on
//                                         the marching-cubes surface and on the dual-contouring surface, int64 counts in front
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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
static void put(std::FILE* f, const T* p, size_t count)
{
	const long long n = static_cast<long long>(count);
	std::fwrite(&n, sizeof(n), 1, f);
	if (n) { std::fwrite(p, sizeof(T), count, f); }
}

int main(int argc, char** argv)
{
	require(argc == 3, "usage: test_meshpts <points.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open points");
	int n = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "read point count");
	std::vector<float> pos(3 * n), nrm(3 * n);
	require(std::fread(pos.data(), sizeof(float), pos.size(), in) == pos.size() &&
	            std::fread(nrm.data(), sizeof(float), nrm.size(), in) == nrm.size(),
	        "read points");
	std::fclose(in);

	const long               count = 5000;
	const unsigned long long seed  = 9;
	const std::vector<int>   sizes = {40, 36, 32};
	std::unique_ptr<fi::GpuLatticeField> field = fi::gpu_sdf_from_points(sizes, fi::Weights(), n, pos.data(), nrm.data(), nullptr);
	std::vector<float> p[2], q[2], p1, q1;
	require(!field->iso_surface_points(0.0f, false, count, seed, &p[0], &q[0]), "iso_surface_points before a solve fails");
	field->set_levels(3, true);
	const std::vector<float> x = field->solve(0, 1e-6f);
	require(x.size() == field->num_unknowns(), "solve");

	for (int dual = 0; dual < 2; ++dual) {
		require(field->iso_surface_points(0.0f, dual != 0, count, seed, &p[dual], &q[dual]), dual ? "points on the dual contour" : "points on the iso-surface");
		require(p[dual].size() == 3 * static_cast<size_t>(count) && q[dual].size() == p[dual].size(), "... three floats a point");
		bool unit = true;
		for (size_t k = 0; k + 2 < q[dual].size(); k += 3) {
			const double l = std::sqrt(double(q[dual][k]) * q[dual][k] + double(q[dual][k + 1]) * q[dual][k + 1] + double(q[dual][k + 2]) * q[dual][k + 2]);
			unit = unit && std::fabs(l - 1.0) < 1e-6;
		}
		require(unit, "... with unit normals");
		require(field->iso_surface_points(0.0f, dual != 0, count, seed, &p1, nullptr) && same_bits(p1, p[dual]), "without normals: the same positions");
		require(field->iso_surface_points(0.0f, dual != 0, count, seed + 1, &p1, &q1) && !same_bits(p1, p[dual]), "another seed: other points");
		require(field->iso_surface_points(0.0f, dual != 0, 0, seed, &p1, &q1) && p1.empty() && q1.empty(), "no points asked: none given");
		require(!field->iso_surface_points(0.0f, dual != 0, -1, seed, &p1, &q1), "n = -1 is refused");
		require(!field->iso_surface_points(1.0e6f, dual != 0, count, seed, &p1, &q1), "an empty surface has nothing to sample");
	}

	// the C ABI on a device field, every array in device memory
	float* dx = nullptr;
	require(hipMalloc(reinterpret_cast<void**>(&dx), x.size() * sizeof(float)) == hipSuccess, "hipMalloc field");
	require(hipMemcpy(dx, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess, "upload field");
	fi_mesh* m = nullptr;
	require(fi_iso_extract_field(dx, 3, sizes.data(), 0.0f, FI_DEVICE, &m) == FI_OK, "fi_iso_extract_field from device");
	long nv = 0, np = 0;
	require(fi_mesh_info(m, &nv, &np, nullptr) == FI_OK && nv > 0 && np > 0, "fi_mesh_info");
	float *    dp = nullptr, *dn = nullptr, *dd = nullptr;
	long long* di = nullptr;
	require(hipMalloc(reinterpret_cast<void**>(&dp), 3 * count * sizeof(float)) == hipSuccess &&
	            hipMalloc(reinterpret_cast<void**>(&dn), 3 * count * sizeof(float)) == hipSuccess &&
	            hipMalloc(reinterpret_cast<void**>(&di), count * sizeof(long long)) == hipSuccess &&
	            hipMalloc(reinterpret_cast<void**>(&dd), nv * sizeof(float)) == hipSuccess,
	        "hipMalloc outputs");
	require(fi_mesh_sample(m, count, seed, FI_SAMPLE_NORMALS_VERTEX, dp, dn, di, FI_DEVICE) == FI_OK, "fi_mesh_sample into device memory");
	std::vector<float>     p3(3 * count), q3(3 * count), vd(nv);
	std::vector<long long> i3(count);
	require(hipMemcpy(p3.data(), dp, p3.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess &&
	            hipMemcpy(q3.data(), dn, q3.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess &&
	            hipMemcpy(i3.data(), di, i3.size() * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess,
	        "download them");
	require(same_bits(p3, p[0]) && same_bits(q3, q[0]), "the C ABI's points = iso_surface_points'");
	bool ascending = i3[0] >= 0 && i3[count - 1] < np;
	for (long k = 1; k < count; ++k) { ascending = ascending && i3[k - 1] <= i3[k]; }
	require(ascending, "... in ascending primitive order");
	require(fi_mesh_sample(m, count, seed, FI_SAMPLE_NORMALS_FACE, dp, dn, nullptr, FI_DEVICE) == FI_OK &&
	            hipMemcpy(q3.data(), dn, q3.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess && !same_bits(q3, q[0]),
	        "face normals differ from interpolated vertex normals");
	require(fi_mesh_sample(m, count, seed, 2, dp, dn, nullptr, FI_DEVICE) == FI_ERR_INVALID, "normals mode 2 is refused");

	fi_surface* s = nullptr;
	require(fi_surface_from_mesh(&s, m) == FI_OK, "fi_surface_from_mesh");
	fi_deviation of_samples{}, of_vertices{};
	require(fi_mesh_deviation(m, s, count, seed, INFINITY, &of_samples, &of_vertices, dd, FI_DEVICE) == FI_OK, "fi_mesh_deviation of the mesh from itself");
	require(of_samples.queries == count && of_samples.counted == count && of_vertices.queries == nv && of_vertices.counted == nv,
	        "... every sample and every vertex counted");
	// (the samples are fp32 roundings of points of the surface, at coordinates below 64: a few ulps of 64)
	require(of_samples.max <= 4 * 7.63e-6 && of_vertices.max <= 4 * 7.63e-6 && of_samples.mean <= of_samples.rms && of_samples.rms <= of_samples.max,
	        "... all of them on the surface");
	require(hipMemcpy(vd.data(), dd, vd.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess, "download the vertex distances");
	double top = 0.0;
	for (float d : vd) { top = d > top ? d : top; }
	require(top == of_vertices.max, "... the largest vertex distance is of_vertices.max");
	require(fi_mesh_deviation(m, s, -1, seed, INFINITY, &of_samples, &of_vertices, dd, FI_DEVICE) == FI_ERR_INVALID, "samples = -1 is refused");
	fi_surface_destroy(s);
	fi_mesh_destroy(m);
	hipFree(dp);
	hipFree(dn);
	hipFree(di);
	hipFree(dd);
	hipFree(dx);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, x.data(), x.size());
	for (int dual = 0; dual < 2; ++dual) {
		put(out, p[dual].data(), p[dual].size());
		put(out, q[dual].data(), q[dual].size());
	}
	std::fclose(out);
	std::printf("all meshpts checks passed\n");
	return 0;
}
