// The descriptors and their matching of the C++ drop-in against the C ABI.
//   test_feature <points.bin> <out.bin>   points.bin: int32 n, then n positions and n normals (3 floats each).
//                                         describe_points and match_features are called on them and held to the bytes of
//                                         fi_points_describe and fi_feature_match, with host and with device pointers.
//                                         out.bin: the features, the valid bytes, the matches of the first half's
//                                         descriptors among the second half's and their distances; int64 counts in front
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
	require(argc == 3, "usage: test_feature <points.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open points");
	int n = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 1, "read point count");
	std::vector<float> pos(3 * n), nrm(3 * n);
	require(std::fread(pos.data(), sizeof(float), pos.size(), in) == pos.size() &&
	            std::fread(nrm.data(), sizeof(float), nrm.size(), in) == nrm.size(),
	        "read points and normals");
	std::fclose(in);

	// descriptors
	std::vector<float>         feat, f2(33 * static_cast<size_t>(n));
	std::vector<unsigned char> valid, v2(n);
	require(fi::describe_points(pos, nrm, &feat, &valid, 16) && feat.size() == f2.size() && static_cast<int>(valid.size()) == n,
	        "describe_points");
	fi_points* set = nullptr;
	require(fi_points_create(&set, 3, n, pos.data(), FI_HOST) == FI_OK, "fi_points_create");
	require(fi_points_describe(set, nrm.data(), 16, INFINITY, f2.data(), v2.data(), FI_HOST) == FI_OK && same(feat, f2) && same(valid, v2),
	        "... = fi_points_describe");
	long described = 0;
	for (unsigned char b : valid) { described += b; }
	require(described > n / 2, "... most points have a descriptor");
	std::vector<float> alone;
	require(fi::describe_points(pos, nrm, &alone, nullptr, 16) && same(alone, feat), "... the features alone");
	float*         dn = on_device(nrm);
	float*         df = on_device(f2);
	unsigned char* dv = on_device(v2);
	require(fi_points_describe(set, dn, 16, INFINITY, df, dv, FI_DEVICE) == FI_OK && same(from_device(df, feat.size()), feat) &&
	            same(from_device(dv, n), valid),
	        "device pointers: features and valid");
	require(fi_points_describe(set, dn, 16, INFINITY, df, nullptr, FI_DEVICE) == FI_OK && same(from_device(df, feat.size()), feat),
	        "device pointers: no valid bytes asked for");
	std::vector<float> empty;
	require(fi::describe_points(empty, empty, &alone) && alone.empty(), "an empty cloud");
	require(!fi::describe_points(pos, nrm, nullptr) && !fi::describe_points(pos, empty, &alone) && !fi::describe_points(pos, nrm, &alone, nullptr, 0) &&
	            !fi::describe_points(pos, nrm, &alone, nullptr, 33) && !fi::describe_points(pos, nrm, &alone, nullptr, 8, -1.0f),
	        "... a null output, missing normals, k of 0 and 33, a negative distance are refused");
	fi_points_destroy(set);

	// matching: the first half's descriptors among the second half's
	const int          na = n / 2, nb = n - na;
	std::vector<float> a(feat.begin(), feat.begin() + 33 * static_cast<size_t>(na)), b(feat.begin() + 33 * static_cast<size_t>(na), feat.end());
	std::vector<unsigned char> va(valid.begin(), valid.begin() + na), vb(valid.begin() + na, valid.end());
	std::vector<long long>     idx, i2(na);
	std::vector<float>         dist, d2(na);
	require(fi::match_features(33, a, b, &idx, &dist, va, vb) && static_cast<int>(idx.size()) == na, "match_features");
	require(fi_feature_match(33, na, a.data(), va.data(), nb, b.data(), vb.data(), i2.data(), d2.data(), FI_HOST) == FI_OK && same(idx, i2) &&
	            same(dist, d2),
	        "... = fi_feature_match");
	bool sound = true;
	for (int i = 0; i < na; ++i) { sound = sound && (va[i] ? idx[i] >= 0 && idx[i] < nb && vb[idx[i]] : idx[i] == -1 && std::isinf(dist[i])); }
	require(sound, "... a valid row finds a valid partner, any other row none");
	std::vector<long long> plain;
	require(fi::match_features(33, a, b, &plain) && fi_feature_match(33, na, a.data(), nullptr, nb, b.data(), nullptr, i2.data(), nullptr, FI_HOST) == FI_OK &&
	            same(plain, i2),
	        "no masks, no distances");
	float*         da  = on_device(a);
	float*         db  = on_device(b);
	unsigned char* dva = on_device(va);
	unsigned char* dvb = on_device(vb);
	long long*     di  = on_device(i2);
	float*         dd  = on_device(d2);
	require(fi_feature_match(33, na, da, dva, nb, db, dvb, di, dd, FI_DEVICE) == FI_OK && same(from_device(di, na), idx) &&
	            same(from_device(dd, na), dist),
	        "device pointers: indices and distances");
	require(!fi::match_features(0, a, b, &idx) && !fi::match_features(65, a, b, &idx) && !fi::match_features(33, a, b, nullptr) &&
	            !fi::match_features(32, a, b, &idx) && !fi::match_features(33, a, b, &idx, nullptr, vb, vb),
	        "... a width of 0 and 65, a null output, rows that do not divide, a mask of the wrong length are refused");
	require(fi::match_features(33, a, b, &idx, &dist, va, vb), "match_features again");
	hipFree(dd), hipFree(di), hipFree(dvb), hipFree(dva), hipFree(db), hipFree(da), hipFree(dv), hipFree(df), hipFree(dn);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, feat.data(), feat.size());
	put(out, valid.data(), valid.size());
	put(out, idx.data(), idx.size());
	put(out, dist.data(), dist.size());
	std::fclose(out);
	std::printf("all feature checks passed\n");
	return 0;
}
