// dump_rows: runs the row builders of <field_interpolation/field_interpolation.hpp> over a file of cases and writes what they
// made.  Written against the public headers alone, so the same source builds against this repository's drop-in
// (include/ + libfield_interpolation.so) and against the reference's headers and its compiled assembly
// (oracle/_ref/libfi_ref.so): tests/test_reference_rows.py requires the two outputs to be byte-identical.
//
//   dump_rows CASES OUT            rows, right-hand sides, returns and operator<< text (host code only)
//   dump_rows --device CASES OUT   generate_error_map and upscale_field instead (the drop-in runs these on the GPU), and,
//                                  where the headers have it, the returns of GpuLatticeField's single-constraint calls
//
// Case file: whitespace-separated tokens; every float is the hexadecimal form of its 32 bits.
//   NCASES, then per case:  name D sizes[D] weights[8] value_kernel gradient_kernel model_last print
//                           NPTS has_normals has_weights positions[NPTS*D] normals[..] point_weights[..]
//                           NOPS, per op: kind kernel pos[D] gradient[D] value weight
//                           NX x[NX]
//   NUPSCALES, then per pair: D small[D] large[D] field[prod(small)]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include <field_interpolation/field_interpolation.hpp>
#if defined(__has_include)
#if __has_include(<field_interpolation/gpu_field.hpp>)
#include <field_interpolation/gpu_field.hpp>
#define DUMP_ROWS_HAS_GPU_FIELD 1
#endif
#endif

namespace fi = field_interpolation;

static float read_float(std::istream& in)
{
	std::string tok;
	in >> tok;
	const uint32_t bits = static_cast<uint32_t>(std::stoul(tok, nullptr, 16));
	float f;
	std::memcpy(&f, &bits, sizeof f);
	return f;
}

static std::vector<float> read_floats(std::istream& in, size_t n)
{
	std::vector<float> v(n);
	for (auto& x : v) { x = read_float(in); }
	return v;
}

static unsigned bits_of(float f)
{
	uint32_t bits;
	std::memcpy(&bits, &f, sizeof bits);
	return bits;
}

static void write_floats(std::FILE* out, const char* tag, const std::vector<float>& v)
{
	std::fprintf(out, "%s %zu", tag, v.size());
	for (float x : v) { std::fprintf(out, " %08x", bits_of(x)); }
	std::fprintf(out, "\n");
}

int main(int argc, char** argv)
{
	const bool device = argc > 1 && std::strcmp(argv[1], "--device") == 0;
	if (argc != (device ? 4 : 3)) {
		std::fprintf(stderr, "usage: dump_rows [--device] CASES OUT\n");
		return 2;
	}
	std::ifstream in(argv[device ? 2 : 1]);
	std::FILE* out = std::fopen(argv[device ? 3 : 2], "w");
	if (!in || !out) {
		std::fprintf(stderr, "dump_rows: cannot open the files\n");
		return 2;
	}
	int num_cases = 0;
	in >> num_cases;
	for (int c = 0; c < num_cases; ++c) {
		std::string name;
		int D = 0;
		in >> name >> D;
		std::vector<int> sizes(D);
		for (int& s : sizes) { in >> s; }
		fi::Weights w;
		w.data_pos = read_float(in);
		w.data_gradient = read_float(in);
		w.model_0 = read_float(in);
		w.model_1 = read_float(in);
		w.model_2 = read_float(in);
		w.model_3 = read_float(in);
		w.model_4 = read_float(in);
		w.gradient_smoothness = read_float(in);
		int vk = 0, gk = 0, model_last = 0, print = 0, npts = 0, has_normals = 0, has_weights = 0;
		in >> vk >> gk >> model_last >> print >> npts >> has_normals >> has_weights;
		w.value_kernel = static_cast<fi::ValueKernel>(vk);
		w.gradient_kernel = static_cast<fi::GradientKernel>(gk);
		const std::vector<float> pos = read_floats(in, static_cast<size_t>(npts) * D);
		const std::vector<float> nrm = read_floats(in, has_normals ? static_cast<size_t>(npts) * D : 0);
		const std::vector<float> pw = read_floats(in, has_weights ? npts : 0);

		fi::LatticeField field(sizes);
		if (!model_last) { fi::add_field_constraints(&field, w); }
		if (npts > 0) {
			fi::add_points(&field, w.data_pos, w.value_kernel, w.data_gradient, w.gradient_kernel, npts, pos.data(),
			               has_normals ? nrm.data() : nullptr, has_weights ? pw.data() : nullptr);
		}
		int num_ops = 0;
		in >> num_ops;
		std::vector<int> returns(num_ops);
#ifdef DUMP_ROWS_HAS_GPU_FIELD
		std::vector<int> gpu_returns(device ? num_ops : 0);
		std::unique_ptr<fi::GpuLatticeField> gpu(device ? new fi::GpuLatticeField(sizes) : nullptr);
		if (gpu) { gpu->add_field_constraints(w); }
#endif
		for (int k = 0; k < num_ops; ++k) {
			int kind = 0, kernel = 0;
			in >> kind >> kernel;
			const std::vector<float> p = read_floats(in, D), g = read_floats(in, D);
			const float value = read_float(in), weight = read_float(in);
			if (kind == 0) {
				returns[k] = fi::add_value_constraint(&field, p.data(), value, weight);
			} else if (kind == 1) {
				returns[k] = fi::add_value_constraint_nearest_neighbor(&field, p.data(), g.data(), value, weight);
			} else {
				returns[k] = fi::add_gradient_constraint(&field, p.data(), g.data(), weight, static_cast<fi::GradientKernel>(kernel));
			}
#ifdef DUMP_ROWS_HAS_GPU_FIELD
			if (gpu && kind == 0) {
				gpu_returns[k] = gpu->add_value_constraint(p.data(), value, weight);
			} else if (gpu && kind == 1) {
				gpu_returns[k] = gpu->add_value_constraint_nearest_neighbor(p.data(), g.data(), value, weight);
			} else if (gpu) {
				gpu_returns[k] = gpu->add_gradient_constraint(p.data(), g.data(), weight, static_cast<fi::GradientKernel>(kernel));
			}
#endif
		}
		if (model_last) { fi::add_field_constraints(&field, w); }
		int nx = 0;
		in >> nx;
		const std::vector<float> x = read_floats(in, nx);
		if (!in) {
			std::fprintf(stderr, "dump_rows: case %d is cut short\n", c);
			return 2;
		}

		std::fprintf(out, "case %s\n", name.c_str());
		if (device) {
			write_floats(out, "errmap", fi::generate_error_map(field.eq.triplets, x, field.eq.rhs));
#ifdef DUMP_ROWS_HAS_GPU_FIELD
			std::fprintf(out, "gpureturns %d", num_ops);
			for (int r : gpu_returns) { std::fprintf(out, " %d", r); }
			std::fprintf(out, "\n");
#endif
			continue;
		}
		std::fprintf(out, "counts %zu %zu\n", field.eq.rhs.size(), field.eq.triplets.size());
		for (const fi::Triplet& t : field.eq.triplets) { std::fprintf(out, "t %d %d %08x\n", t.row, t.col, bits_of(t.value)); }
		write_floats(out, "rhs", field.eq.rhs);
		std::fprintf(out, "returns %d", num_ops);
		for (int r : returns) { std::fprintf(out, " %d", r); }
		std::fprintf(out, "\n");
		if (print) {
			std::ostringstream os;
			os << field.eq;
			std::fprintf(out, "text %zu\n%s", os.str().size(), os.str().c_str());
		}
	}
	int num_upscales = 0;
	in >> num_upscales;
	for (int j = 0; j < num_upscales; ++j) {
		int D = 0;
		in >> D;
		std::vector<int> small(D), large(D);
		size_t n = 1;
		for (int& s : small) { in >> s; n *= static_cast<size_t>(s); }
		for (int& s : large) { in >> s; }
		const std::vector<float> f = read_floats(in, n);
		if (!in) {
			std::fprintf(stderr, "dump_rows: upscale %d is cut short\n", j);
			return 2;
		}
		if (device) { write_floats(out, "upscale", fi::upscale_field(f.data(), small, large)); }
	}
	return std::fclose(out) == 0 ? 0 : 1;
}
