// The clustering call of GpuLatticeField against the C ABI.
//   test_cluster <points.bin> <out.bin>   points.bin: int32 n, then n positions and n normals (3 floats each, lattice units)
//                                         for a 32 x 32 x 32 lattice.  The points become the data points of a field (no solve
//                                         is needed); cluster_points is called on them and held to the C ABI's bytes on a
//                                         fi_points of the same cloud, with host and with device pointers, and the table of
//                                         fi_cluster_measure is taken both ways.
//                                         out.bin: labels and core bytes at min_points 1 and 4, the two stats structs as bytes,
//                                         the rows of the first labelling as bytes; int64 counts in front
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

template <typename T>
static bool same(const std::vector<T>& a, const std::vector<T>& b)
{
	return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

template <typename T>
static T* on_device(const std::vector<T>& v)
{
	T* d = nullptr;
	require(hipMalloc(reinterpret_cast<void**>(&d), (v.size() + 1) * sizeof(T)) == hipSuccess &&
	            hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess,
	        "upload");
	return d;
}

template <typename T>
static std::vector<T> from_device(const T* d, size_t count)
{
	std::vector<T> v(count);
	require(hipMemcpy(v.data(), d, count * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess, "download");
	return v;
}

int main(int argc, char** argv)
{
	require(argc == 3, "usage: test_cluster <points.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open points");
	int n = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "read point count");
	std::vector<float> pos(3 * n), nrm(3 * n);
	require(std::fread(pos.data(), sizeof(float), pos.size(), in) == pos.size() &&
	            std::fread(nrm.data(), sizeof(float), nrm.size(), in) == nrm.size(),
	        "read points");
	std::fclose(in);

	const std::vector<int> sizes = {32, 32, 32};
	std::unique_ptr<fi::GpuLatticeField> field = fi::gpu_sdf_from_points(sizes, fi::Weights(), n, pos.data(), nrm.data(), nullptr);
	fi_points* set = nullptr;
	require(fi_points_create(&set, 3, n, pos.data(), FI_HOST) == FI_OK, "fi_points_create");

	// Euclidean clusters, then DBSCAN
	std::vector<int>           labels1, labels4, l2(n);
	std::vector<unsigned char> core1, core4, c2(n);
	fi::ClusterStats           stats1{}, stats4{};
	fi_cluster_stats           s2{};
	require(field->cluster_points(1.5f, 1, &labels1, &core1, &stats1) && static_cast<int>(labels1.size()) == n, "cluster_points, min_points 1");
	require(fi_points_cluster(set, 1.5f, 1, l2.data(), c2.data(), &s2, FI_HOST) == FI_OK && same(labels1, l2) && same(core1, c2) &&
	            std::memcmp(&stats1, &s2, sizeof(s2)) == 0,
	        "... = fi_points_cluster");
	require(stats1.clusters >= 2 && stats1.core == n && stats1.border == 0 && stats1.noise == 0 && stats1.non_finite == 0,
	        "... every point is core, at least two clusters");
	require(field->cluster_points(0.6f, 4, &labels4, &core4, &stats4), "cluster_points, min_points 4");
	require(fi_points_cluster(set, 0.6f, 4, l2.data(), c2.data(), &s2, FI_HOST) == FI_OK && same(labels4, l2) && same(core4, c2) &&
	            std::memcmp(&stats4, &s2, sizeof(s2)) == 0,
	        "... = fi_points_cluster");
	require(stats4.core + stats4.border + stats4.noise == n && stats4.border > 0 && stats4.noise > 0, "... core, border and noise add up");
	std::vector<int> only;
	require(field->cluster_points(1.5f, 1, &only) && same(only, labels1), "... labels alone");
	require(!field->cluster_points(-1.0f, 1, &only) && !field->cluster_points(NAN, 1, &only) &&
	            !field->cluster_points(std::numeric_limits<float>::infinity(), 1, &only) && !field->cluster_points(1.0f, 0, &only) &&
	            !field->cluster_points(1.0f, 1, nullptr),
	        "... a negative, NaN or infinite eps, min_points 0, a null output are refused");

	// the same call with device pointers
	int*           dl = on_device(l2);
	unsigned char* dc = on_device(c2);
	require(fi_points_cluster(set, 0.6f, 4, dl, dc, &s2, FI_DEVICE) == FI_OK && same(from_device(dl, n), labels4) &&
	            same(from_device(dc, n), core4) && std::memcmp(&stats4, &s2, sizeof(s2)) == 0,
	        "device pointers: labels, core, stats");

	// the table
	std::vector<fi_cluster_row> rows(stats1.clusters), rows2(stats1.clusters);
	require(fi_cluster_measure(3, n, pos.data(), labels1.data(), core1.data(), stats1.clusters, rows.data(), FI_HOST) == FI_OK, "fi_cluster_measure");
	long members = 0;
	for (const fi_cluster_row& r : rows) { members += r.count; }
	require(members == n && rows[0].core == rows[0].count, "... the rows count every point");
	float* dp = on_device(pos);
	require(hipMemcpy(dl, labels1.data(), sizeof(int) * n, hipMemcpyHostToDevice) == hipSuccess &&
	            hipMemcpy(dc, core1.data(), n, hipMemcpyHostToDevice) == hipSuccess,
	        "upload the labelling");
	require(fi_cluster_measure(3, n, dp, dl, dc, stats1.clusters, rows2.data(), FI_DEVICE) == FI_OK &&
	            std::memcmp(rows.data(), rows2.data(), rows.size() * sizeof(fi_cluster_row)) == 0,
	        "device pointers: the table");
	require(fi_cluster_measure(3, n, pos.data(), labels1.data(), nullptr, stats1.clusters - 1, rows2.data(), FI_HOST) == FI_ERR_INVALID,
	        "... a label out of range is refused");
	hipFree(dl), hipFree(dc), hipFree(dp);
	fi_points_destroy(set);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, labels1.data(), labels1.size());
	put(out, core1.data(), core1.size());
	put(out, labels4.data(), labels4.size());
	put(out, core4.data(), core4.size());
	put(out, reinterpret_cast<const unsigned char*>(&stats1), sizeof(stats1));
	put(out, reinterpret_cast<const unsigned char*>(&stats4), sizeof(stats4));
	put(out, reinterpret_cast<const unsigned char*>(rows.data()), rows.size() * sizeof(fi_cluster_row));
	std::fclose(out);
	std::printf("all cluster checks passed\n");
	return 0;
}
