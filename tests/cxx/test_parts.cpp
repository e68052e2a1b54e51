// GpuLatticeField::iso_surface_parts on a solved 3-D SDF.
//   test_parts <points.bin> <out.bin>   points.bin: int32 n, then n positions and n normals (3 floats each, lattice units) for a
//                                       40 x 36 x 32 lattice; solves with the V-cycle, extracts the iso-surface of the solution
//                                       with every part kept (which must equal iso_surface) and with only the largest part, for
//                                       both extractors, and walks the C ABI (fi_mesh_parts / _measure / _select) on a device
//                                       field against it.
//                                       out.bin: the solution, then the largest part's vertices, normals, indices, and its row
//                                       as bytes (int64 counts in front)
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
	require(argc == 3, "usage: test_parts <points.bin> <out.bin>");
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
	std::vector<float>        v0, n0, v1, n1, v2, n2;
	std::vector<int>          i0, i1, i2;
	std::vector<fi::MeshPart> all, one;
	require(!field->iso_surface_parts(0.0f, false, -1, 0.0, &v0, &i0, &n0, &all), "iso_surface_parts before a solve fails");
	field->set_levels(3, true);
	const std::vector<float> x = field->solve(0, 1e-6f);
	require(x.size() == field->num_unknowns(), "solve");

	for (int dual = 0; dual < 2; ++dual) {
		require(dual ? field->dual_contour(0.0f, &v0, &i0, &n0) : field->iso_surface(0.0f, &v0, &i0, &n0), "the whole mesh");
		require(field->iso_surface_parts(0.0f, dual != 0, -1, 0.0, &v1, &i1, &n1, &all), "iso_surface_parts, everything kept");
		require(same_bits(v1, v0) && same_bits(n1, n0) && same_bits(i1, i0), "... is the whole mesh");
		long long prims = 0, verts = 0;
		size_t    best = 0;
		for (size_t c = 0; c < all.size(); ++c) {
			prims += all[c].primitives;
			verts += all[c].vertices;
			if (all[c].size > all[best].size) { best = c; }
		}
		require(!all.empty() && prims * 3 == static_cast<long long>(i0.size()) && verts * 3 == static_cast<long long>(v0.size()),
		        "the parts hold every primitive and every vertex");
		require(field->iso_surface_parts(0.0f, dual != 0, 1, 0.0, &v2, &i2, &n2, &one), "iso_surface_parts, the largest part");
		require(one.size() == 1 && std::memcmp(&one[0], &all[best], sizeof(fi::MeshPart)) == 0, "... has the largest part's row");
		require(static_cast<long long>(i2.size()) == 3 * one[0].primitives && static_cast<long long>(v2.size()) == 3 * one[0].vertices &&
		            n2.size() == v2.size(),
		        "... and its primitives and vertices");
		require(field->iso_surface_parts(0.0f, dual != 0, -1, 2.0 * all[best].size, &v1, &i1, nullptr, &all) && v1.empty() && i1.empty() &&
		            all.empty(),
		        "a min_size nothing reaches leaves an empty mesh");
		if (dual) { break; }

		// the C ABI on a device field, labels into device memory
		float* dx = nullptr;
		require(hipMalloc(reinterpret_cast<void**>(&dx), x.size() * sizeof(float)) == hipSuccess, "hipMalloc field");
		require(hipMemcpy(dx, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess, "upload field");
		fi_mesh* m = nullptr;
		require(fi_iso_extract_field(dx, 3, sizes.data(), 0.0f, FI_DEVICE, &m) == FI_OK, "fi_iso_extract_field from device");
		long count = 0, nv = 0, np = 0;
		require(fi_mesh_info(m, &nv, &np, nullptr) == FI_OK && 3 * nv == static_cast<long>(v0.size()), "fi_mesh_info");
		int* dl = nullptr;
		require(hipMalloc(reinterpret_cast<void**>(&dl), (nv + np) * sizeof(int)) == hipSuccess, "hipMalloc labels");
		require(fi_mesh_parts(m, &count, dl, dl + nv, FI_DEVICE) == FI_OK, "fi_mesh_parts into device memory");
		std::vector<int> labels(nv + np);
		require(hipMemcpy(labels.data(), dl, labels.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess, "download labels");
		bool in_range = true;
		for (int l : labels) { in_range = in_range && 0 <= l && l < count; }
		require(in_range, "every label names a part");
		std::vector<fi_mesh_part> rows(count);
		require(fi_mesh_measure(m, count, rows.data(), nullptr) == FI_OK && std::memcmp(&rows[best], &one[0], sizeof(fi_mesh_part)) == 0,
		        "fi_mesh_measure");
		std::vector<unsigned char> keep(count, 0);
		keep[best] = 1;
		fi_mesh* k = nullptr;
		require(fi_mesh_select(m, count, keep.data(), &k) == FI_OK, "fi_mesh_select");
		require(fi_mesh_info(k, &nv, &np, nullptr) == FI_OK, "fi_mesh_info of the selection");
		std::vector<float> v3(3 * nv), n3(3 * nv);
		std::vector<int>   i3(3 * np);
		require(fi_mesh_copy(k, v3.data(), n3.data(), i3.data(), nullptr, FI_HOST) == FI_OK, "fi_mesh_copy");
		require(same_bits(v3, v2) && same_bits(n3, n2) && same_bits(i3, i2), "the C ABI's selection = iso_surface_parts'");
		fi_mesh_destroy(k);
		fi_mesh_destroy(m);
		hipFree(dl);
		hipFree(dx);

		std::FILE* out = std::fopen(argv[2], "wb");
		require(out != nullptr, "open output");
		put(out, x.data(), x.size());
		put(out, v2.data(), v2.size());
		put(out, n2.data(), n2.size());
		put(out, i2.data(), i2.size());
		put(out, reinterpret_cast<const unsigned char*>(one.data()), sizeof(fi::MeshPart));
		std::fclose(out);
	}
	std::printf("all parts checks passed\n");
	return 0;
}
