// GpuLatticeField::sample on a solved 3-D SDF, and the device-resident paths of the C ABI beside it.
//   test_sample <points.bin> <out.bin>
// points.bin: int32 n, then n positions and n normals (3 floats each, lattice units), for a 40 x 36 x 32 lattice.
// The program solves, samples the solution in place at the data points (linear and cubic, with gradients), and checks that
// fi_sample on a context and fi_sample_field with every buffer on the device (hipMalloc) give the same results bit for bit
// as the host path.  out.bin: the solution, then linear values and gradients, cubic values and gradients (int64 counts in
// front).
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

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b)
{
	return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

static void put(std::FILE* f, const std::vector<float>& v)
{
	const long long n = static_cast<long long>(v.size());
	std::fwrite(&n, sizeof(n), 1, f);
	if (n) { std::fwrite(v.data(), sizeof(float), v.size(), f); }
}

static float* to_device(const std::vector<float>& h)
{
	void* p = nullptr;
	require(hipMalloc(&p, h.size() * sizeof(float) + 16) == hipSuccess, "hipMalloc");
	require(hipMemcpy(p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess, "upload");
	return static_cast<float*>(p);
}

static std::vector<float> from_device(const float* p, size_t n)
{
	std::vector<float> h(n);
	require(hipMemcpy(h.data(), p, n * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess, "download");
	return h;
}

int main(int argc, char** argv)
{
	require(argc == 3, "usage: test_sample <points.bin> <out.bin>");
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open points");
	int n = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "read point count");
	std::vector<float> pos(3 * n), nrm(3 * n);
	require(std::fread(pos.data(), sizeof(float), pos.size(), in) == pos.size() &&
	            std::fread(nrm.data(), sizeof(float), nrm.size(), in) == nrm.size(),
	        "read points");
	std::fclose(in);
	// and three points outside the lattice
	const float outside[9] = {-1.0f, 1.0f, 1.0f, 1.0f, 36.0f, 1.0f, 1.0f, 1.0f, NAN};
	pos.insert(pos.end(), outside, outside + 9);
	const size_t m = pos.size() / 3;

	const std::vector<int> sizes = {40, 36, 32};
	std::unique_ptr<fi::GpuLatticeField> field =
	    fi::gpu_sdf_from_points(sizes, fi::Weights(), n, pos.data(), nrm.data(), nullptr);
	std::vector<float> v0, g0;
	require(!field->sample(pos, &v0, &g0), "sample before a solve fails");
	const std::vector<float> x = field->solve(0, 1e-6f);
	require(x.size() == field->num_unknowns(), "solve");
	require(field->sample(pos, &v0, &g0) && v0.size() == m && g0.size() == 3 * m, "GpuLatticeField::sample");
	require(std::isnan(v0[m - 1]) && std::isnan(g0[3 * m - 1]), "outside points get NaN");
	std::vector<float> v_only;
	require(field->sample(pos, &v_only) && same_bits(v_only, v0), "without gradients");
	std::vector<float> c0, cg0;
	require(field->sample(pos, &c0, &cg0, true), "cubic");

	// the same field through the C ABI with every buffer on the device
	float* dx = to_device(x);
	float* dp = to_device(pos);
	float *dv = nullptr, *dg = nullptr;
	require(hipMalloc(reinterpret_cast<void**>(&dv), m * sizeof(float)) == hipSuccess &&
	            hipMalloc(reinterpret_cast<void**>(&dg), 3 * m * sizeof(float)) == hipSuccess,
	        "hipMalloc outputs");
	const float nan = NAN;
	for (int mode = FI_SAMPLE_LINEAR; mode <= FI_SAMPLE_CUBIC; ++mode) {
		const std::vector<float>& wv = mode == FI_SAMPLE_LINEAR ? v0 : c0;
		const std::vector<float>& wg = mode == FI_SAMPLE_LINEAR ? g0 : cg0;
		require(fi_sample_field(dx, 3, sizes.data(), static_cast<long>(m), dp, mode, nan, dv, dg, FI_DEVICE) == FI_OK,
		        "fi_sample_field, device buffers");
		require(same_bits(from_device(dv, m), wv) && same_bits(from_device(dg, 3 * m), wg), "device field = solution in place");
		fi_ctx* c = nullptr;
		require(fi_ctx_create(&c, 3, sizes.data(), FI_F32) == FI_OK, "fi_ctx_create");
		require(fi_sample(c, nullptr, static_cast<long>(m), pos.data(), mode, nan, v_only.data(), nullptr, FI_HOST) == FI_ERR_STATE,
		        "fi_sample without a solution: FI_ERR_STATE");
		require(fi_sample(c, dx, static_cast<long>(m), dp, mode, nan, dv, dg, FI_DEVICE) == FI_OK, "fi_sample, device buffers");
		require(same_bits(from_device(dv, m), wv) && same_bits(from_device(dg, 3 * m), wg), "context, device field = in place");
		std::vector<float> hv(m), hg(3 * m);
		require(fi_sample(c, x.data(), static_cast<long>(m), pos.data(), mode, nan, hv.data(), hg.data(), FI_HOST) == FI_OK &&
		            same_bits(hv, wv) && same_bits(hg, wg),
		        "context, host field = in place");
		fi_ctx_destroy(c);
	}
	{
		// fi_upscale_field: the same bytes from host and from device buffers
		const std::vector<int> large = {45, 37, 33};
		const size_t           nl    = 45 * 37 * 33;
		std::vector<float>     up(nl);
		float*                 du = nullptr;
		require(hipMalloc(reinterpret_cast<void**>(&du), nl * sizeof(float)) == hipSuccess, "hipMalloc upscaled");
		require(fi_upscale_field(x.data(), 3, sizes.data(), large.data(), up.data(), FI_HOST) == FI_OK &&
		            fi_upscale_field(dx, 3, sizes.data(), large.data(), du, FI_DEVICE) == FI_OK && same_bits(from_device(du, nl), up) &&
		            up[0] == x[0],
		        "fi_upscale_field, host = device buffers");
		hipFree(du);
	}
	hipFree(dx);
	hipFree(dp);
	hipFree(dv);
	hipFree(dg);

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, x);
	put(out, v0);
	put(out, g0);
	put(out, c0);
	put(out, cg0);
	std::fclose(out);
	std::printf("all sample checks passed\n");
	return 0;
}
