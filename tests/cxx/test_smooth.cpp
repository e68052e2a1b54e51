// GpuLatticeField::iso_surface_smoothed on a solved 3-D SDF.
//   test_smooth <points.bin> <out.bin>   points.bin: int32 n, then n positions and n normals (3 floats each, lattice units) for a
//                                        40 x 36 x 32 lattice; solves with the V-cycle, smooths the iso-surface of the solution
//                                        with both extractors, with and without the largest-part rule, and walks the C ABI
//                                        (fi_mesh_smooth, fi_mesh_normals with device pointers) against it.
//                                        out.bin: the solution, then the vertices, normals and indices of the Taubin result
//                                        (every part, 5 iterations) and of the clamped Laplacian result (largest part, 3
//                                        iterations, max_move 0.25), int64 counts in front
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
	require(argc == 3, "usage: test_smooth <points.bin> <out.bin>");
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
	std::vector<float> v0, n0, vt, nt, vl, nl, v1, n1;
	std::vector<int>   i0, it, il, i1;
	require(!field->iso_surface_smoothed(0.0f, false, 5, 0.5f, -0.53f, 0.0f, -1, 0.0, &v0, &i0, &n0), "iso_surface_smoothed before a solve fails");
	field->set_levels(3, true);
	const std::vector<float> x = field->solve(0, 1e-6f);
	require(x.size() == field->num_unknowns(), "solve");

	for (int dual = 0; dual < 2; ++dual) {
		require(dual ? field->dual_contour(0.0f, &v0, &i0, &n0) : field->iso_surface(0.0f, &v0, &i0, &n0), "the whole mesh");
		require(field->iso_surface_smoothed(0.0f, dual != 0, 5, 0.5f, -0.53f, 0.0f, -1, 0.0, &vt, &it, &nt), "Taubin, 5 iterations");
		require(same_bits(it, i0) && vt.size() == v0.size() && nt.size() == n0.size() && !same_bits(vt, v0), "... the indices stay, the vertices move");
		require(field->iso_surface_smoothed(0.0f, dual != 0, 0, 0.5f, -0.53f, 0.0f, -1, 0.0, &v1, &i1, nullptr) && same_bits(v1, v0) && same_bits(i1, i0),
		        "no iterations: the input's bytes");
		require(field->iso_surface_smoothed(0.0f, dual != 0, 3, 0.5f, 0.0f, 0.25f, 1, 0.0, &vl, &il, &nl), "Laplacian, max_move 0.25, largest part");
		require(!il.empty() && il.size() <= i0.size() && vl.size() == nl.size(), "... is no larger");
		bool unit = true;
		for (size_t k = 0; k + 2 < nl.size(); k += 3) {
			const double l = std::sqrt(double(nl[k]) * nl[k] + double(nl[k + 1]) * nl[k + 1] + double(nl[k + 2]) * nl[k + 2]);
			unit = unit && std::fabs(l - 1.0) < 1e-6;
		}
		require(unit, "... with unit normals");
		require(!field->iso_surface_smoothed(0.0f, dual != 0, -1, 0.5f, -0.53f, 0.0f, -1, 0.0, &v1, &i1, &n1), "iterations -1 is refused");
		require(!field->iso_surface_smoothed(0.0f, dual != 0, 1, 1.5f, -0.53f, 0.0f, -1, 0.0, &v1, &i1, &n1), "lambda 1.5 is refused");
		require(!field->iso_surface_smoothed(0.0f, dual != 0, 1, 0.5f, 0.1f, 0.0f, -1, 0.0, &v1, &i1, &n1), "mu 0.1 is refused");
		require(!field->iso_surface_smoothed(0.0f, dual != 0, 1, 0.5f, 0.0f, -1.0f, -1, 0.0, &v1, &i1, &n1), "max_move -1 is refused");
		if (dual) { break; }

		// the C ABI on a device field, the arrays copied into device memory
		float* dx = nullptr;
		require(hipMalloc(reinterpret_cast<void**>(&dx), x.size() * sizeof(float)) == hipSuccess, "hipMalloc field");
		require(hipMemcpy(dx, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess, "upload field");
		fi_mesh* m = nullptr;
		require(fi_iso_extract_field(dx, 3, sizes.data(), 0.0f, FI_DEVICE, &m) == FI_OK, "fi_iso_extract_field from device");
		long nv = 0, np = 0, sv = 0, sp = 0;
		require(fi_mesh_info(m, &nv, &np, nullptr) == FI_OK && 3 * nv == static_cast<long>(v0.size()), "fi_mesh_info");
		fi_smooth_options opt{};
		opt.iterations = 5;
		opt.lambda     = 0.5f;
		opt.mu         = -0.53f;
		opt.boundary   = FI_SMOOTH_BOUNDARY_FIXED;
		opt.max_move   = 0.0f;
		opt.normals    = FI_SMOOTH_NORMALS_KEEP;
		fi_mesh* s = nullptr;
		require(fi_mesh_smooth(m, &opt, &s) == FI_OK, "fi_mesh_smooth, normals kept");
		require(fi_mesh_info(s, &sv, &sp, nullptr) == FI_OK && sv == nv && sp == np, "fi_mesh_info of the result");
		float *dv = nullptr, *dn = nullptr;
		require(hipMalloc(reinterpret_cast<void**>(&dv), 3 * nv * sizeof(float)) == hipSuccess &&
		            hipMalloc(reinterpret_cast<void**>(&dn), 3 * nv * sizeof(float)) == hipSuccess,
		        "hipMalloc vertices and normals");
		require(fi_mesh_copy(s, dv, dn, nullptr, nullptr, FI_DEVICE) == FI_OK, "fi_mesh_copy into device memory");
		std::vector<float> v3(3 * nv), n3(3 * nv), n4(3 * nv);
		require(hipMemcpy(v3.data(), dv, v3.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess &&
		            hipMemcpy(n3.data(), dn, n3.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess,
		        "download them");
		require(same_bits(v3, vt) && same_bits(n3, n0), "the C ABI's vertices = iso_surface_smoothed's, the kept normals = the extractor's");
		fi_mesh* sn = nullptr;
		require(fi_mesh_normals(s, &sn) == FI_OK && fi_mesh_copy(sn, v3.data(), n4.data(), nullptr, nullptr, FI_HOST) == FI_OK, "fi_mesh_normals of it");
		require(same_bits(v3, vt) && same_bits(n4, nt), "... = the normals iso_surface_smoothed recomputed");
		opt.boundary = 3;
		fi_mesh* bad = nullptr;
		require(fi_mesh_smooth(m, &opt, &bad) == FI_ERR_INVALID && bad == nullptr, "boundary 3 is refused");
		fi_mesh_destroy(sn);
		fi_mesh_destroy(s);
		fi_mesh_destroy(m);
		hipFree(dv);
		hipFree(dn);
		hipFree(dx);

		std::FILE* out = std::fopen(argv[2], "wb");
		require(out != nullptr, "open output");
		put(out, x.data(), x.size());
		put(out, vt.data(), vt.size());
		put(out, nt.data(), nt.size());
		put(out, it.data(), it.size());
		put(out, vl.data(), vl.size());
		put(out, nl.data(), nl.size());
		put(out, il.data(), il.size());
		std::fclose(out);
	}
	std::printf("all smooth checks passed\n");
	return 0;
}
