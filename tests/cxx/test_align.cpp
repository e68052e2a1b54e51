// The coarse alignment of the C++ drop-in against the C ABI.
//   test_align <pairs.bin> <out.bin>   pairs.bin: int32 n_s, n_t, m, then the source and target points (3 floats each) and
//                                      the m source and m target indices (int64).  align_correspondences is called on them
//                                      and held to the bytes of fi_align_correspondences, with host and with device pointers.
//                                      out.bin: the result as bytes and the inlier bytes; int64 counts in front
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
	require(argc == 3, "usage: test_align <pairs.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open pairs");
	int counts[3] = {0, 0, 0};
	require(std::fread(counts, sizeof(int), 3, in) == 3 && counts[0] > 0 && counts[1] > 0 && counts[2] > 2, "read counts");
	const int              ns = counts[0], nt = counts[1], m = counts[2];
	std::vector<float>     src(3 * ns), tgt(3 * nt);
	std::vector<long long> si(m), ti(m);
	require(std::fread(src.data(), sizeof(float), src.size(), in) == src.size() && std::fread(tgt.data(), sizeof(float), tgt.size(), in) == tgt.size() &&
	            std::fread(si.data(), sizeof(long long), m, in) == static_cast<size_t>(m) &&
	            std::fread(ti.data(), sizeof(long long), m, in) == static_cast<size_t>(m),
	        "read points and indices");
	std::fclose(in);
	static_assert(sizeof(fi::Alignment) == sizeof(fi_alignment), "Alignment mirrors fi_alignment");

	fi::Alignment              got{};
	std::vector<unsigned char> inliers, i2(m);
	require(fi::align_correspondences(src, tgt, si, ti, 0.05f, &got, &inliers) && static_cast<int>(inliers.size()) == m, "align_correspondences");
	fi_align_options opt{};
	opt.threshold  = 0.05f;
	opt.similarity = 0.9f;
	opt.max_trials = 100000;
	opt.confidence = 0.999;
	fi_alignment r2{};
	require(fi_align_correspondences(ns, src.data(), nt, tgt.data(), m, si.data(), ti.data(), &opt, &r2, i2.data(), FI_HOST) == FI_OK &&
	            same(inliers, i2) && std::memcmp(&got, &r2, sizeof(r2)) == 0,
	        "... = fi_align_correspondences");
	long counted = 0;
	for (unsigned char b : inliers) { counted += b; }
	require(got.found == 1 && got.inliers == counted && got.pairs == m && got.live <= m && got.trials % FI_ALIGN_BATCH == 0 && got.valid > 0,
	        "... found, and the mask holds what the result counts");
	require(got.transform[12] == 0.0 && got.transform[13] == 0.0 && got.transform[14] == 0.0 && got.transform[15] == 1.0 && got.rms < 0.05,
	        "... a rigid motion in homogeneous form");
	fi::Alignment alone{};
	require(fi::align_correspondences(src, tgt, si, ti, 0.05f, &alone) && std::memcmp(&alone, &got, sizeof(got)) == 0, "... the result alone");
	fi::Alignment seeded{};
	opt.similarity = 0.0f;
	opt.max_trials = 3000;
	opt.confidence = 0.0;
	opt.seed       = 5;
	require(fi::align_correspondences(src, tgt, si, ti, 0.05f, &seeded, &inliers, 0.0f, 3000, 0.0, 5) &&
	            fi_align_correspondences(ns, src.data(), nt, tgt.data(), m, si.data(), ti.data(), &opt, &r2, i2.data(), FI_HOST) == FI_OK &&
	            same(inliers, i2) && std::memcmp(&seeded, &r2, sizeof(r2)) == 0 && seeded.trials == 3000 && seeded.valid <= 3000,
	        "no edge test, every trial, a seed");
	require(!fi::align_correspondences(src, tgt, si, ti, -1.0f, &got) && !fi::align_correspondences(src, tgt, si, ti, NAN, &got) &&
	            !fi::align_correspondences(src, tgt, si, ti, 0.05f, nullptr) && !fi::align_correspondences(src, tgt, si, ti, 0.05f, &got, nullptr, 1.5f) &&
	            !fi::align_correspondences(src, tgt, si, ti, 0.05f, &got, nullptr, 0.9f, 0) &&
	            !fi::align_correspondences(src, tgt, si, ti, 0.05f, &got, nullptr, 0.9f, 100, 1.0) &&
	            !fi::align_correspondences(src, tgt, si, std::vector<long long>(ti.begin(), ti.end() - 1), 0.05f, &got),
	        "... a bad threshold, a null result, similarity 1.5, no trials, confidence 1, unequal index lists are refused");
	require(fi::align_correspondences(src, tgt, si, ti, 0.05f, &got, &inliers), "align_correspondences again");

	// the same call with device pointers
	opt            = fi_align_options{};
	opt.threshold  = 0.05f;
	opt.similarity = 0.9f;
	opt.max_trials = 100000;
	opt.confidence = 0.999;
	float*         ds  = on_device(src);
	float*         dt  = on_device(tgt);
	long long*     dsi = on_device(si);
	long long*     dti = on_device(ti);
	unsigned char* di  = on_device(i2);
	require(fi_align_correspondences(ns, ds, nt, dt, m, dsi, dti, &opt, &r2, di, FI_DEVICE) == FI_OK && same(from_device(di, m), inliers) &&
	            std::memcmp(&got, &r2, sizeof(r2)) == 0,
	        "device pointers: the result and the inliers");
	require(fi_align_correspondences(ns, ds, nt, dt, m, dsi, dti, &opt, &r2, nullptr, FI_DEVICE) == FI_OK && std::memcmp(&got, &r2, sizeof(r2)) == 0,
	        "device pointers: no inlier bytes asked for");
	hipFree(di), hipFree(dti), hipFree(dsi), hipFree(dt), hipFree(ds);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, reinterpret_cast<const unsigned char*>(&got), sizeof(got));
	put(out, inliers.data(), inliers.size());
	std::fclose(out);
	std::printf("all align checks passed\n");
	return 0;
}
