// fi_ref_capi.cpp -- C ABI over the public headers of the reference's field_interpolation library.  TEST INFRASTRUCTURE ONLY.
//
// Linked with the reference's own assembly file and the Eigen-free head of its sparse_linear.cpp (add_equation and
// operator<<) into oracle/_ref/libfi_ref.so; see oracle/Makefile.  Nothing in this file restates the reference: every
// entry forwards to a function its headers declare.  Every entry returns a status (0 fine, 1 a reference check failed --
// the logging stand-in throws where the reference would abort --, 2 any other exception) and never lets an exception out.
#include <algorithm>
#include <cstring>
#include <exception>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "field_interpolation.hpp"

namespace fi = field_interpolation;

namespace {

thread_local std::string g_error;

template <typename F>
int guarded(F&& body)
{
	try {
		body();
		return 0;
	} catch (const std::runtime_error& e) {
		g_error = e.what();
		return 1;
	} catch (const std::exception& e) {
		g_error = e.what();
		return 2;
	} catch (...) {
		g_error = "unknown exception";
		return 2;
	}
}

fi::LatticeField* field(void* h) { return static_cast<fi::LatticeField*>(h); }

}  // namespace

extern "C" {

struct fir_weights {  // the members of field_interpolation::Weights, in order
	float data_pos, data_gradient, model_0, model_1, model_2, model_3, model_4, gradient_smoothness;
	int   value_kernel, gradient_kernel;
};

static fi::Weights to_weights(const fir_weights* w)
{
	fi::Weights out;
	out.data_pos = w->data_pos;
	out.data_gradient = w->data_gradient;
	out.model_0 = w->model_0;
	out.model_1 = w->model_1;
	out.model_2 = w->model_2;
	out.model_3 = w->model_3;
	out.model_4 = w->model_4;
	out.gradient_smoothness = w->gradient_smoothness;
	out.value_kernel = static_cast<fi::ValueKernel>(w->value_kernel);
	out.gradient_kernel = static_cast<fi::GradientKernel>(w->gradient_kernel);
	return out;
}

const char* fir_last_error() { return g_error.c_str(); }

int fir_field_new(int ndim, const int* sizes, void** out)
{
	return guarded([&] { *out = new fi::LatticeField(std::vector<int>(sizes, sizes + ndim)); });
}

int fir_field_free(void* h)
{
	return guarded([&] { delete field(h); });
}

int fir_counts(void* h, long* num_rows, long* num_triplets)
{
	return guarded([&] {
		*num_rows = static_cast<long>(field(h)->eq.rhs.size());
		*num_triplets = static_cast<long>(field(h)->eq.triplets.size());
	});
}

int fir_get(void* h, int* rows, int* cols, float* vals, float* rhs)
{
	return guarded([&] {
		const fi::LinearEquation& eq = field(h)->eq;
		for (size_t k = 0; k < eq.triplets.size(); ++k) {
			rows[k] = eq.triplets[k].row;
			cols[k] = eq.triplets[k].col;
			vals[k] = eq.triplets[k].value;
		}
		for (size_t k = 0; k < eq.rhs.size(); ++k) { rhs[k] = eq.rhs[k]; }
	});
}

int fir_add_equation(void* h, float weight, float rhs, int n, const int* cols, const float* coef)
{
	return guarded([&] {
		// add_equation takes an initializer_list: one call per length the reference's own callers use
		fi::LinearEquation* eq = &field(h)->eq;
		const fi::Weight w{weight};
		const fi::Rhs r{rhs};
		switch (n) {
		case 1: fi::add_equation(eq, w, r, {{cols[0], coef[0]}}); break;
		case 2: fi::add_equation(eq, w, r, {{cols[0], coef[0]}, {cols[1], coef[1]}}); break;
		case 3: fi::add_equation(eq, w, r, {{cols[0], coef[0]}, {cols[1], coef[1]}, {cols[2], coef[2]}}); break;
		case 4:
			fi::add_equation(eq, w, r, {{cols[0], coef[0]}, {cols[1], coef[1]}, {cols[2], coef[2]}, {cols[3], coef[3]}});
			break;
		case 5:
			fi::add_equation(eq, w, r,
			                 {{cols[0], coef[0]}, {cols[1], coef[1]}, {cols[2], coef[2]}, {cols[3], coef[3]}, {cols[4], coef[4]}});
			break;
		default: throw std::invalid_argument("fir_add_equation: 1 to 5 terms");
		}
	});
}

int fir_add_field_constraints(void* h, const fir_weights* w)
{
	return guarded([&] { fi::add_field_constraints(field(h), to_weights(w)); });
}

int fir_add_points(void* h, float vw, int vk, float gw, int gk, int n, const float* pos, const float* normals, const float* pw)
{
	return guarded([&] {
		fi::add_points(field(h), vw, static_cast<fi::ValueKernel>(vk), gw, static_cast<fi::GradientKernel>(gk), n, pos, normals,
		               pw);
	});
}

int fir_sdf_from_points(int ndim, const int* sizes, const fir_weights* w, int n, const float* pos, const float* normals,
                        const float* pw, void** out)
{
	return guarded([&] {
		*out = new fi::LatticeField(
		    fi::sdf_from_points(std::vector<int>(sizes, sizes + ndim), to_weights(w), n, pos, normals, pw));
	});
}

int fir_add_value_constraint(void* h, const float* pos, float value, float weight, int* accepted)
{
	return guarded([&] { *accepted = fi::add_value_constraint(field(h), pos, value, weight) ? 1 : 0; });
}

int fir_add_value_constraint_nearest_neighbor(void* h, const float* pos, const float* gradient, float value, float weight,
                                              int* accepted)
{
	return guarded([&] { *accepted = fi::add_value_constraint_nearest_neighbor(field(h), pos, gradient, value, weight) ? 1 : 0; });
}

int fir_add_gradient_constraint(void* h, const float* pos, const float* gradient, float weight, int kernel, int* accepted)
{
	return guarded([&] {
		*accepted = fi::add_gradient_constraint(field(h), pos, gradient, weight, static_cast<fi::GradientKernel>(kernel)) ? 1 : 0;
	});
}

int fir_error_map(void* h, long ncols, const float* solution, float* out)
{
	return guarded([&] {
		const std::vector<float> x(solution, solution + ncols);
		const std::vector<float> heat = fi::generate_error_map(field(h)->eq.triplets, x, field(h)->eq.rhs);
		if (static_cast<long>(heat.size()) != ncols) { throw std::logic_error("generate_error_map: unexpected length"); }
		std::memcpy(out, heat.data(), heat.size() * sizeof(float));
	});
}

int fir_upscale_field(const float* small, int ndim_small, const int* small_sizes, int ndim_large, const int* large_sizes,
                      long capacity, float* out)
{
	return guarded([&] {
		const std::vector<float> large = fi::upscale_field(small, std::vector<int>(small_sizes, small_sizes + ndim_small),
		                                                   std::vector<int>(large_sizes, large_sizes + ndim_large));
		if (static_cast<long>(large.size()) > capacity) { throw std::logic_error("upscale_field: unexpected length"); }
		std::memcpy(out, large.data(), large.size() * sizeof(float));
	});
}

// operator<< of the field's system into buf (not terminated); *needed is the full length either way.
int fir_print(void* h, char* buf, long capacity, long* needed)
{
	return guarded([&] {
		std::ostringstream os;
		os << field(h)->eq;
		const std::string text = os.str();
		*needed = static_cast<long>(text.size());
		if (buf && capacity > 0) { std::memcpy(buf, text.data(), static_cast<size_t>(std::min<long>(capacity, *needed))); }
	});
}

}  // extern "C"
