// GpuLatticeField::solve_robust / point_residuals on 2-D value data with gross errors.
//   test_robust <points.bin> <out.bin>
// points.bin: int32 n, then n positions (2 floats each, lattice units) and n values, for a 64 x 64 lattice with model_2 = 3.
// The program solves the plain fit (fp32), takes every point's residual against it, then runs five robust rounds.
// out.bin: the plain field, the residuals, the robust field, the weight factors (int64 counts in front), then the iterations
// of the plain solve and of all solves of the loop (two int64).
#include <cstdio>
#include <cstdlib>
#include <vector>

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
static void put(std::FILE* f, const std::vector<T>& v)
{
	const long long n = static_cast<long long>(v.size());
	std::fwrite(&n, sizeof(n), 1, f);
	if (n) { std::fwrite(v.data(), sizeof(T), v.size(), f); }
}

int main(int argc, char** argv)
{
	if (argc != 3) { return 2; }
	std::FILE* in = std::fopen(argv[1], "rb");
	require(in != nullptr, "open points");
	int n = 0;
	require(std::fread(&n, sizeof(n), 1, in) == 1 && n > 0, "point count");
	std::vector<float> pos(2 * static_cast<size_t>(n)), val(static_cast<size_t>(n));
	require(std::fread(pos.data(), sizeof(float), pos.size(), in) == pos.size(), "positions");
	require(std::fread(val.data(), sizeof(float), val.size(), in) == val.size(), "values");
	std::fclose(in);

	fi::GpuLatticeField field({64, 64});
	fi::Weights w;
	w.model_2 = 3.0f;
	field.add_field_constraints(w);
	std::vector<float> none;
	require(!field.point_residuals(&none), "no residuals without points");
	int accepted = 0;
	for (int i = 0; i < n; ++i) { accepted += field.add_value_constraint(&pos[2 * i], val[i], 1.0f) ? 1 : 0; }
	require(accepted == n, "every point accepted");
	std::vector<float> residuals;
	require(!field.point_residuals(&residuals), "no residuals before the first solve");

	const std::vector<float> plain = field.solve(0, 1e-6f);
	require(plain.size() == 64 * 64, "plain solve");
	const long long it_plain = field.last_iterations();
	require(field.point_residuals(&residuals) && residuals.size() == static_cast<size_t>(n), "residuals");

	fi::RobustOptions opt;
	opt.loss   = fi::RobustOptions::Loss::kHuber;
	opt.rounds = 5;
	std::vector<float> omega;
	const std::vector<float> robust = field.solve_robust(opt, 0, 1e-6f, &omega);
	require(robust.size() == 64 * 64 && omega.size() == static_cast<size_t>(n), "robust solve");
	const long long it_all = field.last_iterations();
	require(it_all > it_plain, "the loop counts the iterations of all its solves");

	std::FILE* out = std::fopen(argv[2], "wb");
	require(out != nullptr, "open output");
	put(out, plain);
	put(out, residuals);
	put(out, robust);
	put(out, omega);
	std::fwrite(&it_plain, sizeof(it_plain), 1, out);
	std::fwrite(&it_all, sizeof(it_all), 1, out);
	std::fclose(out);
	std::printf("all robust checks passed\n");
	return 0;
}
