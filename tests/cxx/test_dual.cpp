// GpuLatticeField::dual_contour on a solved 3-D SDF, and the dc:: drop-in (include/field_interpolation/dual_contouring_2d.hpp).
//   test_dual solve <points.bin> <out.bin>   points.bin: int32 n, then n positions and n normals (3 floats each, lattice units)
//                                            for a 40 x 36 x 32 lattice; solves with the V-cycle, dual-contours the solution on
//                                            the device and checks fi_dual_contour_field from a device pointer against it.
//                                            out.bin: the solution, vertices, normals, indices (int64 counts in front)
//   test_dual dc <case.bin> <out.bin>        case.bin: int64 width, height, has_gradients, then width * height distances and,
//                                            if given, the gradients; calls dc::calculate_gradients where none are given, then
//                                            dc::dual_contouring_2d twice into the same vectors (the second call appends).
//                                            out.bin: the first call's vertices and segments
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include <fi_hip.h>

#include <field_interpolation/dual_contouring_2d.hpp>
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

static int solve_mode(const char* in_path, const char* out_path)
{
	std::FILE* in = std::fopen(in_path, "rb");
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
	std::vector<float> v0, n0;
	std::vector<int>   i0;
	require(!field->dual_contour(0.0f, &v0, &i0, &n0), "dual_contour before a solve fails");
	field->set_levels(3, true);
	const std::vector<float> x = field->solve(0, 1e-6f);
	require(x.size() == field->num_unknowns(), "solve");
	require(field->dual_contour(0.0f, &v0, &i0, &n0), "GpuLatticeField::dual_contour");
	require(!v0.empty() && i0.size() % 3 == 0 && n0.size() == v0.size(), "a non-empty triangle mesh");
	std::vector<float> bad(5);
	require(!field->dual_contour(0.0f, &v0, &i0, nullptr, &bad), "gradients of the wrong length are refused");

	float* dx = nullptr;
	require(hipMalloc(reinterpret_cast<void**>(&dx), x.size() * sizeof(float)) == hipSuccess, "hipMalloc field");
	require(hipMemcpy(dx, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess, "upload field");
	fi_mesh* m = nullptr;
	require(fi_dual_contour_field(dx, nullptr, 3, sizes.data(), 0.0f, FI_DEVICE, &m) == FI_OK, "fi_dual_contour_field from device");
	long nv = 0, np = 0;
	int  vpp = 0;
	require(fi_mesh_info(m, &nv, &np, &vpp) == FI_OK && vpp == 3, "fi_mesh_info");
	std::vector<float> v1(3 * nv), n1(3 * nv);
	std::vector<int>   i1(3 * np);
	require(fi_mesh_copy(m, v1.data(), n1.data(), i1.data(), nullptr, FI_HOST) == FI_OK, "fi_mesh_copy");
	fi_mesh_destroy(m);
	hipFree(dx);
	require(same_bits(v1, v0) && same_bits(n1, n0) && same_bits(i1, i0), "device field = solution in place");

	std::FILE* out = std::fopen(out_path, "wb");
	require(out != nullptr, "open output");
	put(out, x.data(), x.size());
	put(out, v0.data(), v0.size());
	put(out, n0.data(), n0.size());
	put(out, i0.data(), i0.size());
	std::fclose(out);
	std::printf("all dual checks passed\n");
	return 0;
}

static int dc_mode(const char* in_path, const char* out_path)
{
	std::FILE* in = std::fopen(in_path, "rb");
	require(in != nullptr, "open case");
	long long hdr[3] = {0, 0, 0};
	require(std::fread(hdr, sizeof(long long), 3, in) == 3, "read header");
	const size_t w = static_cast<size_t>(hdr[0]), h = static_cast<size_t>(hdr[1]);
	std::vector<float>   d(w * h);
	std::vector<dc::Vec2> g(w * h);
	require(std::fread(d.data(), sizeof(float), d.size(), in) == d.size(), "read distances");
	if (hdr[2]) {
		require(std::fread(g.data(), sizeof(dc::Vec2), g.size(), in) == g.size(), "read gradients");
	} else {
		dc::calculate_gradients(g.data(), w, h, d.data());
	}
	std::fclose(in);
	std::vector<dc::Vec2> verts;
	std::vector<unsigned> segs;
	dc::dual_contouring_2d(&verts, &segs, w, h, d.data(), g.data());
	require(!verts.empty() && segs.size() % 2 == 0, "dc::dual_contouring_2d");
	const size_t nv = verts.size(), ns = segs.size();
	dc::dual_contouring_2d(&verts, &segs, w, h, d.data(), g.data());
	bool appended = verts.size() == 2 * nv && segs.size() == 2 * ns;
	for (size_t i = 0; appended && i < ns; ++i) { appended = segs[ns + i] == segs[i] + nv; }
	require(appended, "a second call appends, its indices after the first's vertices");
	std::FILE* out = std::fopen(out_path, "wb");
	require(out != nullptr, "open output");
	put(out, reinterpret_cast<const float*>(verts.data()), 2 * nv);
	put(out, segs.data(), ns);
	std::fclose(out);
	std::printf("all dc checks passed\n");
	return 0;
}

int main(int argc, char** argv)
{
	require(argc == 4, "usage: test_dual solve|dc <in.bin> <out.bin>");
	return std::string(argv[1]) == "solve" ? solve_mode(argv[2], argv[3]) : dc_mode(argv[2], argv[3]);
}
