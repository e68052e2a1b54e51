// GpuLatticeField::iso_surface_simplified on a solved 3-D SDF.
//   test_simplify <points.bin> <out.bin>   points.bin: int32 n, then n positions and n normals (3 floats each, lattice units) for a
//                                          40 x 36 x 32 lattice; solves with the V-cycle, simplifies the iso-surface of the
//                                          solution with both extractors and both placements, with and without the largest-part
//                                          rule, and walks the C ABI (fi_mesh_simplify with device pointers) against it.
//                                          out.bin: the solution, then the vertices, normals and indices of the quadric result
//                                          at cell 2 (every part) and of the mean result at cell 3 (largest part), int64 counts
//                                          in front
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
	require(argc == 3, "usage: test_simplify <points.bin> <out.bin>");
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
	std::vector<float> v0, n0, vq, nq, vm, nm, v1, n1;
	std::vector<int>   i0, iq, im, i1;
	require(!field->iso_surface_simplified(0.0f, false, 2.0f, FI_SIMPLIFY_QUADRIC, -1, 0.0, &v0, &i0, &n0),
	        "iso_surface_simplified before a solve fails");
	field->set_levels(3, true);
	const std::vector<float> x = field->solve(0, 1e-6f);
	require(x.size() == field->num_unknowns(), "solve");

	for (int dual = 0; dual < 2; ++dual) {
		require(dual ? field->dual_contour(0.0f, &v0, &i0, &n0) : field->iso_surface(0.0f, &v0, &i0, &n0), "the whole mesh");
		require(field->iso_surface_simplified(0.0f, dual != 0, 2.0f, FI_SIMPLIFY_QUADRIC, -1, 0.0, &vq, &iq, &nq), "quadric, cell 2");
		require(!iq.empty() && iq.size() < i0.size() / 2 && vq.size() == nq.size() && vq.size() < v0.size() / 2, "... is less than half the size");
		bool in_range = true;
		for (int i : iq) { in_range = in_range && 0 <= i && 3 * static_cast<size_t>(i) < vq.size(); }
		require(in_range, "... with indices in range");
		require(field->iso_surface_simplified(0.0f, dual != 0, 3.0f, FI_SIMPLIFY_MEAN, 1, 0.0, &vm, &im, &nm), "mean, cell 3, largest part");
		require(!im.empty() && im.size() < iq.size(), "... is smaller still");
		require(!field->iso_surface_simplified(0.0f, dual != 0, 0.0f, FI_SIMPLIFY_QUADRIC, -1, 0.0, &v1, &i1, &n1), "cell 0 is refused");
		require(!field->iso_surface_simplified(0.0f, dual != 0, 2.0f, 2, -1, 0.0, &v1, &i1, &n1), "placement 2 is refused");
		// a cell below the vertex spacing changes nothing but the numbering (the extractors' vertices are used and ordered by key
		// = by z, y, x of their lattice edge, not by their own coordinates)
		require(field->iso_surface_simplified(0.0f, dual != 0, 1e-4f, FI_SIMPLIFY_MEAN, -1, 0.0, &v1, &i1, nullptr) && i1.size() <= i0.size() &&
		            v1.size() <= v0.size(),
		        "a tiny cell");
		if (dual) { break; }

		// the C ABI on a device field, the vertex map into device memory
		float* dx = nullptr;
		require(hipMalloc(reinterpret_cast<void**>(&dx), x.size() * sizeof(float)) == hipSuccess, "hipMalloc field");
		require(hipMemcpy(dx, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess, "upload field");
		fi_mesh* m = nullptr;
		require(fi_iso_extract_field(dx, 3, sizes.data(), 0.0f, FI_DEVICE, &m) == FI_OK, "fi_iso_extract_field from device");
		long nv = 0, np = 0, cv = 0, cp = 0;
		require(fi_mesh_info(m, &nv, &np, nullptr) == FI_OK && 3 * nv == static_cast<long>(v0.size()), "fi_mesh_info");
		int* dmap = nullptr;
		require(hipMalloc(reinterpret_cast<void**>(&dmap), nv * sizeof(int)) == hipSuccess, "hipMalloc vertex map");
		fi_mesh* c = nullptr;
		require(fi_mesh_simplify(m, 2.0f, nullptr, FI_SIMPLIFY_QUADRIC, dmap, FI_DEVICE, &c) == FI_OK, "fi_mesh_simplify, map on the device");
		require(fi_mesh_info(c, &cv, &cp, nullptr) == FI_OK, "fi_mesh_info of the result");
		std::vector<float> v3(3 * cv), n3(3 * cv);
		std::vector<int>   i3(3 * cp), map(nv), hmap(nv);
		require(fi_mesh_copy(c, v3.data(), n3.data(), i3.data(), nullptr, FI_HOST) == FI_OK, "fi_mesh_copy");
		require(same_bits(v3, vq) && same_bits(n3, nq) && same_bits(i3, iq), "the C ABI's result = iso_surface_simplified's");
		require(hipMemcpy(map.data(), dmap, map.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess, "download the map");
		bool in_map = true;
		long mapped = 0;
		for (int k : map) {
			in_map = in_map && -1 <= k && k < cv;
			mapped += k >= 0;
		}
		require(in_map && mapped > nv / 2, "the map names output vertices (-1: a cluster whose primitives all collapsed)");
		fi_mesh* c2 = nullptr;
		const float zero[3] = {0.0f, 0.0f, 0.0f};
		require(fi_mesh_simplify(m, 2.0f, zero, FI_SIMPLIFY_QUADRIC, hmap.data(), FI_HOST, &c2) == FI_OK && same_bits(hmap, map),
		        "the map on the host, an explicit zero origin");
		fi_mesh_destroy(c2);
		fi_mesh_destroy(c);
		fi_mesh_destroy(m);
		hipFree(dmap);
		hipFree(dx);

		std::FILE* out = std::fopen(argv[2], "wb");
		require(out != nullptr, "open output");
		put(out, x.data(), x.size());
		put(out, vq.data(), vq.size());
		put(out, nq.data(), nq.size());
		put(out, iq.data(), iq.size());
		put(out, vm.data(), vm.size());
		put(out, nm.data(), nm.size());
		put(out, im.data(), im.size());
		std::fclose(out);
	}
	std::printf("all simplify checks passed\n");
	return 0;
}
