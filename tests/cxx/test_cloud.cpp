// The point-cloud cleaning calls of GpuLatticeField and the free thin_points against the C ABI.
//   test_cloud <points.bin> <out.bin>   points.bin: int32 n, then n positions and n normals (3 floats each, lattice units) for a
//                                       32 x 32 x 32 lattice, then int32 m and m queries (3 floats each).  The points become
//                                       the data points of a field (no solve is needed); every wrapper is called on them and
//                                       held to the C ABI's bytes on a fi_points of the same cloud, with host and with device
//                                       pointers.
//                                       out.bin: the radius counts; mean, kth and counts of the neighbour distances; the two
//                                       masks; the stats struct as bytes; the thinned positions, normals, counts, indices and
//                                       the cell map; int64 counts in front
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
	require(argc == 3, "usage: test_cloud <points.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open points");
	int n = 0, m = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "read point count");
	std::vector<float> pos(3 * n), nrm(3 * n);
	require(std::fread(pos.data(), sizeof(float), pos.size(), in) == pos.size() &&
	            std::fread(nrm.data(), sizeof(float), nrm.size(), in) == nrm.size(),
	        "read points");
	require(std::fread(&m, sizeof(m), 1, in) == 1 && m > 0, "read query count");
	std::vector<float> q(3 * m);
	require(std::fread(q.data(), sizeof(float), q.size(), in) == q.size(), "read queries");
	std::fclose(in);

	const std::vector<int> sizes = {32, 32, 32};
	std::unique_ptr<fi::GpuLatticeField> field = fi::gpu_sdf_from_points(sizes, fi::Weights(), n, pos.data(), nrm.data(), nullptr);
	fi_points* set = nullptr;
	require(fi_points_create(&set, 3, n, pos.data(), FI_HOST) == FI_OK, "fi_points_create");
	const float inf = std::numeric_limits<float>::infinity();

	// radius counts
	std::vector<int> counts, c2(m);
	require(field->radius_count(q, 1.5f, &counts, 6) && static_cast<int>(counts.size()) == m, "radius_count");
	require(fi_points_radius_count(set, m, q.data(), 1.5f, 6, c2.data(), FI_HOST) == FI_OK && same(counts, c2), "... = fi_points_radius_count");
	require(field->radius_count(q, 1.5f, &c2) && !same(counts, c2), "... without a limit some counts are larger");
	require(!field->radius_count(q, -1.0f, &c2) && !field->radius_count(q, 1.0f, &c2, 0) && !field->radius_count(q, 1.0f, nullptr),
	        "... a negative radius, a zero limit, a null output are refused");

	// neighbour distances
	std::vector<float> mean, kth, mean2(n), kth2(n);
	std::vector<int>   cnt, cnt2(n);
	require(field->neighbour_distances(12, &mean, &kth, &cnt) && static_cast<int>(mean.size()) == n, "neighbour_distances");
	require(fi_points_neighbour_distances(set, 12, inf, mean2.data(), kth2.data(), cnt2.data(), FI_HOST) == FI_OK && same(mean, mean2) &&
	            same(kth, kth2) && same(cnt, cnt2),
	        "... = fi_points_neighbour_distances");
	std::vector<float> only;
	require(field->neighbour_distances(12, nullptr, &only) && same(only, kth), "... kth alone");
	require(!field->neighbour_distances(12, nullptr) && !field->neighbour_distances(33, &only) && !field->neighbour_distances(0, &only),
	        "... no output, k = 33, k = 0 are refused");

	// the masks
	std::vector<unsigned char> stat_keep, radius_keep, k2(n);
	fi::OutlierStats           stats{};
	fi_outlier_stats           s2{};
	long                       kept = -1, kept2 = -1;
	require(field->statistical_outliers(12, 1.0f, &stat_keep, &stats), "statistical_outliers");
	require(fi_points_outliers_statistical(set, 12, inf, 1.0f, k2.data(), &s2, FI_HOST) == FI_OK && same(stat_keep, k2) &&
	            std::memcmp(&stats, &s2, sizeof(s2)) == 0,
	        "... = fi_points_outliers_statistical");
	long on = 0;
	for (unsigned char b : stat_keep) { on += b; }
	require(stats.counted == n && stats.kept == on && on < n && stats.threshold > stats.mean, "... the stats count the mask");
	require(!field->statistical_outliers(12, -1.0f, &stat_keep) && !field->statistical_outliers(12, 1.0f, nullptr),
	        "... a negative ratio, a null mask are refused");
	require(field->radius_outliers(1.5f, 2, &radius_keep, &kept), "radius_outliers");
	require(fi_points_outliers_radius(set, 1.5f, 2, k2.data(), &kept2, FI_HOST) == FI_OK && same(radius_keep, k2) && kept == kept2,
	        "... = fi_points_outliers_radius");
	require(!field->radius_outliers(1.5f, 0, &radius_keep) && !field->radius_outliers(NAN, 2, &radius_keep), "... min_neighbours 0, a NaN radius are refused");

	// the same calls with device pointers
	float*         dq  = on_device(q);
	int*           dc  = on_device(c2);
	float*         dm  = on_device(mean2);
	unsigned char* dk  = on_device(k2);
	require(fi_points_radius_count(set, m, dq, 1.5f, 6, dc, FI_DEVICE) == FI_OK && same(from_device(dc, m), counts), "device pointers: counts");
	require(fi_points_neighbour_distances(set, 12, inf, dm, nullptr, nullptr, FI_DEVICE) == FI_OK && same(from_device(dm, n), mean),
	        "device pointers: mean");
	require(fi_points_outliers_statistical(set, 12, inf, 1.0f, dk, &s2, FI_DEVICE) == FI_OK && same(from_device(dk, n), stat_keep) &&
	            std::memcmp(&stats, &s2, sizeof(s2)) == 0,
	        "device pointers: the statistical mask");
	require(fi_points_outliers_radius(set, 1.5f, 2, dk, &kept2, FI_DEVICE) == FI_OK && same(from_device(dk, n), radius_keep) && kept2 == kept,
	        "device pointers: the radius mask");

	// thinning
	std::vector<float>     tp, tn, tp2(pos.size()), tn2(pos.size());
	std::vector<int>       tc, map, tc2(n), map2(n);
	std::vector<long long> ti, ti2(n);
	const std::vector<float> origin = {0.1f, 0.2f, 0.3f};
	require(fi::thin_points(3, pos, 0.75f, &tp, nrm, &tn, std::vector<float>(), nullptr, origin, false, &tc, &ti, &map), "thin_points");
	long cells = 0;
	require(fi_cloud_thin(3, n, pos.data(), nrm.data(), nullptr, 0.75f, origin.data(), FI_THIN_MEAN, tp2.data(), tn2.data(), nullptr, tc2.data(),
	                      ti2.data(), map2.data(), &cells, FI_HOST) == FI_OK,
	        "fi_cloud_thin");
	tp2.resize(3 * cells), tn2.resize(3 * cells), tc2.resize(cells), ti2.resize(cells);
	require(cells > 0 && cells < n && same(tp, tp2) && same(tn, tn2) && same(tc, tc2) && same(ti, ti2) && same(map, map2), "... the same bytes");
	{
		// host memory, 65 points (one 64-lane wave and one more) in fewer cells than points: only num_out rows of the five
		// per-cell outputs are the call's to write, the rows behind them keep what the caller had there
		const int          few = 65;
		const float        mark = -12345.0f;
		std::vector<float> val(few, 2.0f), sp(3 * few, mark), sn(3 * few, mark), sv(few, mark);
		std::vector<int>   sc(few, -7), smap(few, -7);
		std::vector<long long> si(few, -7);
		long               got = 0;
		require(n >= few && fi_cloud_thin(3, few, pos.data(), nrm.data(), val.data(), 16.0f, origin.data(), FI_THIN_MEAN, sp.data(), sn.data(),
		                                  sv.data(), sc.data(), si.data(), smap.data(), &got, FI_HOST) == FI_OK &&
		            got > 0 && got < few,
		        "fi_cloud_thin, 65 points in fewer cells");
		bool written = true, kept_mark = true;
		for (int c = 0; c < few; ++c) {
			const bool mine = c < got;
			const bool marked = sp[3 * c] == mark && sp[3 * c + 1] == mark && sp[3 * c + 2] == mark && sn[3 * c] == mark &&
			                    sn[3 * c + 1] == mark && sn[3 * c + 2] == mark && sv[c] == mark && sc[c] == -7 && si[c] == -7;
			if (mine) { written = written && sc[c] > 0 && si[c] >= 0 && sv[c] == 2.0f && sp[3 * c] != mark; }
			if (!mine) { kept_mark = kept_mark && marked; }
			written = written && smap[c] >= 0 && smap[c] < got;
		}
		require(written, "... num_out rows and the whole cell map are written");
		require(kept_mark, "... the rows from num_out on keep the caller's bytes");
	}
	float* dp  = on_device(pos);
	float* dn  = on_device(nrm);
	float* dtp = on_device(pos);
	float* dtn = on_device(pos);
	long   cells2 = 0;
	require(fi_cloud_thin(3, n, dp, dn, nullptr, 0.75f, origin.data(), FI_THIN_MEAN, dtp, dtn, nullptr, nullptr, nullptr, nullptr, &cells2,
	                      FI_DEVICE) == FI_OK &&
	            cells2 == cells && same(from_device(dtp, tp.size()), tp) && same(from_device(dtn, tn.size()), tn),
	        "device pointers: thinning");
	std::vector<float> first;
	require(fi::thin_points(3, pos, 0.75f, &first, std::vector<float>(), nullptr, std::vector<float>(), nullptr, origin, true) &&
	            first.size() == tp.size() && !same(first, tp),
	        "thin_points, the first of a cell");
	require(!fi::thin_points(3, pos, 0.0f, &first) && !fi::thin_points(4, pos, 1.0f, &first) && !fi::thin_points(3, pos, 1.0f, nullptr),
	        "... a zero cell, four dimensions, a null output are refused");
	hipFree(dq), hipFree(dc), hipFree(dm), hipFree(dk), hipFree(dp), hipFree(dn), hipFree(dtp), hipFree(dtn);
	fi_points_destroy(set);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, counts.data(), counts.size());
	put(out, mean.data(), mean.size());
	put(out, kth.data(), kth.size());
	put(out, cnt.data(), cnt.size());
	put(out, stat_keep.data(), stat_keep.size());
	put(out, radius_keep.data(), radius_keep.size());
	put(out, reinterpret_cast<const unsigned char*>(&stats), sizeof(stats));
	put(out, tp.data(), tp.size());
	put(out, tn.data(), tn.size());
	put(out, tc.data(), tc.size());
	put(out, ti.data(), ti.size());
	put(out, map.data(), map.size());
	std::fclose(out);
	std::printf("all cloud checks passed\n");
	return 0;
}
