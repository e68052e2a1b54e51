// GpuLatticeField::register_points on a solved 3-D SDF.
//   test_register <points.bin> <out.bin>   points.bin: int32 n, then n positions and n normals (3 floats each, lattice units) for a
//                                          40 x 36 x 32 lattice, then int32 m and m positions of the cloud to register; solves
//                                          with the V-cycle, registers the cloud to the iso-surface of the solution with both
//                                          extractors, and walks the C ABI (fi_mesh_register, fi_points_register with device
//                                          pointers) against it.
//                                          out.bin: the solution; the result structs of the marching-cubes and the dual-contouring
//                                          surface as bytes; the transformed points and distances of the C ABI's call; the result
//                                          struct of the point-set call; int64 counts in front
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
static void put(std::FILE* f, const T* p, size_t count)
{
	const long long n = static_cast<long long>(count);
	std::fwrite(&n, sizeof(n), 1, f);
	if (n) { std::fwrite(p, sizeof(T), count, f); }
}

int main(int argc, char** argv)
{
	require(argc == 3, "usage: test_register <points.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open points");
	int n = 0, m = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "read point count");
	std::vector<float> pos(3 * n), nrm(3 * n);
	require(std::fread(pos.data(), sizeof(float), pos.size(), in) == pos.size() &&
	            std::fread(nrm.data(), sizeof(float), nrm.size(), in) == nrm.size(),
	        "read points");
	require(std::fread(&m, sizeof(m), 1, in) == 1 && m > 0, "read cloud count");
	std::vector<float> cloud(3 * m);
	require(std::fread(cloud.data(), sizeof(float), cloud.size(), in) == cloud.size(), "read cloud");
	std::fclose(in);

	const std::vector<int> sizes = {40, 36, 32};
	std::unique_ptr<fi::GpuLatticeField> field = fi::gpu_sdf_from_points(sizes, fi::Weights(), n, pos.data(), nrm.data(), nullptr);
	fi::RegisterOptions options;
	options.max_iterations = 6;
	std::vector<double> T[2], T1;
	fi::Registration    stats[2], s1;
	require(!field->register_points(0.0f, false, m, cloud.data(), options, &T[0], &stats[0]), "register_points before a solve fails");
	field->set_levels(3, true);
	const std::vector<float> x = field->solve(0, 1e-6f);
	require(x.size() == field->num_unknowns(), "solve");

	for (int dual = 0; dual < 2; ++dual) {
		require(field->register_points(0.0f, dual != 0, m, cloud.data(), options, &T[dual], &stats[dual]),
		        dual ? "register to the dual contour" : "register to the iso-surface");
		require(T[dual].size() == 16 && std::memcmp(T[dual].data(), stats[dual].transform, sizeof(double) * 16) == 0, "... a 4 x 4 transform");
		require(stats[dual].queries == m && stats[dual].counted == m && stats[dual].iterations > 0 && stats[dual].iterations <= 6,
		        "... every point counted");
		require(T[dual][12] == 0.0 && T[dual][13] == 0.0 && T[dual][14] == 0.0 && T[dual][15] == 1.0, "... its last row (0 0 0 1)");
		require(field->register_points(0.0f, dual != 0, m, cloud.data(), options, &T1) && T1 == T[dual], "a second call: the same bytes");
		require(field->register_points(0.0f, dual != 0, 0, nullptr, options, &T1, &s1) && s1.queries == 0 && T1[0] == 1.0 && T1[3] == 0.0,
		        "no points: the identity");
		require(!field->register_points(0.0f, dual != 0, -1, cloud.data(), options, &T1), "n = -1 is refused");
		fi::RegisterOptions bad = options;
		bad.loss                = fi::RegisterOptions::Loss::kTukey;
		require(!field->register_points(0.0f, dual != 0, m, cloud.data(), bad, &T1), "a loss without a scale is refused");
	}

	// the C ABI on a device field, every array in device memory
	float *dx = nullptr, *dc = nullptr, *dp = nullptr, *dd = nullptr;
	require(hipMalloc(reinterpret_cast<void**>(&dx), x.size() * sizeof(float)) == hipSuccess &&
	            hipMalloc(reinterpret_cast<void**>(&dc), cloud.size() * sizeof(float)) == hipSuccess &&
	            hipMalloc(reinterpret_cast<void**>(&dp), cloud.size() * sizeof(float)) == hipSuccess &&
	            hipMalloc(reinterpret_cast<void**>(&dd), m * sizeof(float)) == hipSuccess,
	        "hipMalloc");
	require(hipMemcpy(dx, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
	            hipMemcpy(dc, cloud.data(), cloud.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess,
	        "upload field and cloud");
	fi_mesh* mesh = nullptr;
	require(fi_iso_extract_field(dx, 3, sizes.data(), 0.0f, FI_DEVICE, &mesh) == FI_OK, "fi_iso_extract_field from device");
	fi_surface* surface = nullptr;
	require(fi_surface_from_mesh(&surface, mesh) == FI_OK, "fi_surface_from_mesh");
	fi_register_options opt{FI_REGISTER_PLANE, 6, INFINITY, 1e-6, 1e-6, FI_LOSS_NONE, 0.0f, 0.0f};
	fi_registration     r{}, r2{}, rp{};
	require(fi_mesh_register(mesh, surface, m, dc, &opt, nullptr, &r, dp, dd, FI_DEVICE) == FI_OK, "fi_mesh_register with device pointers");
	require(std::memcmp(&r, &stats[0], sizeof(r)) == 0, "the C ABI's result = register_points'");
	require(fi_mesh_register(mesh, nullptr, m, dc, &opt, nullptr, &r2, nullptr, nullptr, FI_DEVICE) == FI_OK && std::memcmp(&r, &r2, sizeof(r)) == 0,
	        "without an index: the same bytes");
	std::vector<float> moved(cloud.size()), dist(m);
	require(hipMemcpy(moved.data(), dp, moved.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess &&
	            hipMemcpy(dist.data(), dd, dist.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess,
	        "download the transformed points and the distances");
	bool finite = r.rms > 0.0 && std::isfinite(r.rms);
	for (float d : dist) { finite = finite && std::isfinite(d); }
	require(finite, "... every distance finite");
	opt.mode = 2;
	require(fi_mesh_register(mesh, surface, m, dc, &opt, nullptr, &r2, dp, dd, FI_DEVICE) == FI_ERR_INVALID, "mode 2 is refused");
	opt.mode = FI_REGISTER_POINT;
	require(fi_mesh_register(nullptr, surface, m, dc, &opt, nullptr, &r2, nullptr, nullptr, FI_DEVICE) == FI_OK && r2.counted == m,
	        "a surface alone serves FI_REGISTER_POINT");

	// the moved cloud as a point set of its own: the cloud registers to it with a step of nothing
	fi_points* set = nullptr;
	require(fi_points_create(&set, 3, m, dp, FI_DEVICE) == FI_OK, "fi_points_create from device");
	require(fi_points_register(set, nullptr, m, dp, &opt, nullptr, &rp, nullptr, nullptr, FI_DEVICE) == FI_OK, "fi_points_register with device pointers");
	require(rp.counted == m && rp.rms == 0.0 && rp.converged == 1 && rp.iterations == 1, "... a set against itself: converged at once");
	opt.mode = FI_REGISTER_PLANE;
	require(fi_points_register(set, nullptr, m, dp, &opt, nullptr, &r2, nullptr, nullptr, FI_DEVICE) == FI_ERR_INVALID,
	        "FI_REGISTER_PLANE without normals is refused");
	fi_points_destroy(set);
	fi_surface_destroy(surface);
	fi_mesh_destroy(mesh);
	hipFree(dx);
	hipFree(dc);
	hipFree(dp);
	hipFree(dd);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, x.data(), x.size());
	for (int dual = 0; dual < 2; ++dual) { put(out, reinterpret_cast<const unsigned char*>(&stats[dual]), sizeof(stats[dual])); }
	put(out, moved.data(), moved.size());
	put(out, dist.data(), dist.size());
	put(out, reinterpret_cast<const unsigned char*>(&rp), sizeof(rp));
	std::fclose(out);
	std::printf("all register checks passed\n");
	return 0;
}
