// Holds the drop-in's matrix-free path (LinearEquation::recipe, field_interpolation_amd/cxx/recipe.hpp) to the rows that are
// in `eq`.  The program carries its own reference: double-precision least squares and weighted-Jacobi sweeps on eq.triplets
// and eq.rhs exactly as they stand, certified before use (|A^T(Ax-b)|_inf <= 1e-12 |A^T b|_inf, else "reference not
// converged", exit status 3 -- never a library failure).  Prints "ok ..." lines; exits 1 on the first failure.
//   test_recipe host F B.  the note's validation (detail::noted_rows_unchanged) refuses every in-place edit of a noted range
//                          of field F (2d, 3d, hand) and accepts copies and appended rows; with 2d, its throughput.  No device.
//   test_recipe sizing C2's host half alone: every edit moves the reference solution by >= 100 x the tolerance.  No device.
//   test_recipe c1 D   C1. rows re-made from the note == the rows in eq, on the D-dimensional lattice ({96}, {48,40},
//                          {14,12,13}): every solver entry point against the reference, over weights, kernels, point
//                          weights with zeros and point clouds on the lattice's edges.
//   test_recipe c2     C2. edits at indices a sampled checksum would not read are solved, not ignored.
//   test_recipe c3     C3. the cached device context carries nothing from one system to the next.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <field_interpolation/field_interpolation.hpp>
#include <field_interpolation/gpu_field.hpp>
#include <field_interpolation/sparse_linear.hpp>

#include "recipe.hpp"

namespace fi = field_interpolation;
using fi::detail::Segment;

static bool keep_going = false;  // C1: a failed comparison is counted and the remaining cases still print their figures
static int  failures = 0;

static void require(bool ok, const char* what)
{
	if (!ok) {
		std::printf("FAILED: %s\n", what);
		if (!keep_going) { std::exit(1); }
		++failures;
		return;
	}
	std::printf("ok   %s\n", what);
}

// ---- the reference: fp64 on eq.triplets / eq.rhs as they stand -------------------------------------------------------------

// A^T (A x - b) (with_b) or A^T A x, accumulated in T
template <typename T>
static std::vector<T> normal_product(const fi::LinearEquation& eq, const std::vector<double>& x, bool with_b)
{
	std::vector<T> y(eq.rhs.size(), T(0)), g(x.size(), T(0));
	if (with_b) {
		for (size_t i = 0; i < y.size(); ++i) { y[i] = -T(eq.rhs[i]); }
	}
	for (const fi::Triplet& t : eq.triplets) { y[static_cast<size_t>(t.row)] += T(t.value) * T(x[static_cast<size_t>(t.col)]); }
	for (const fi::Triplet& t : eq.triplets) { g[static_cast<size_t>(t.col)] += T(t.value) * y[static_cast<size_t>(t.row)]; }
	return g;
}

struct Normal {  // A^T b and the diagonal of A^T A
	std::vector<double> atb, diag;
	double atb_inf = 0;
};

// The diagonal of A^T A: the sum over the rows of the squared entry in column j, where triplets that name the same (row,
// col) are ONE entry, their sum (Eigen's setFromTriplets; the rows of GradientKernel::kLinearInterpolation name the
// point between two samples twice, +c0 and -c1).
static std::vector<double> normal_diagonal(const fi::LinearEquation& eq, size_t n)
{
	std::vector<size_t> order(eq.triplets.size());
	for (size_t i = 0; i < order.size(); ++i) { order[i] = i; }
	std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
		const fi::Triplet &p = eq.triplets[a], &q = eq.triplets[b];
		return p.row != q.row ? p.row < q.row : p.col < q.col;
	});
	std::vector<double> diag(n, 0.0);
	for (size_t i = 0; i < order.size();) {
		const fi::Triplet& first = eq.triplets[order[i]];
		double entry = 0;
		for (; i < order.size() && eq.triplets[order[i]].row == first.row && eq.triplets[order[i]].col == first.col; ++i) {
			entry += static_cast<double>(eq.triplets[order[i]].value);
		}
		diag[static_cast<size_t>(first.col)] += entry * entry;
	}
	return diag;
}

static Normal normal_of(const fi::LinearEquation& eq, size_t n)
{
	for (const fi::Triplet& t : eq.triplets) {
		if (t.row < 0 || static_cast<size_t>(t.row) >= eq.rhs.size() || t.col < 0 || static_cast<size_t>(t.col) >= n) {
			std::printf("reference: a triplet outside the system (row %d, col %d)\n", t.row, t.col);
			std::exit(3);
		}
	}
	Normal s;
	const std::vector<long double> g = normal_product<long double>(eq, std::vector<double>(n, 0.0), true);
	s.atb.resize(n);
	s.diag = normal_diagonal(eq, n);
	for (size_t j = 0; j < n; ++j) {
		s.atb[j]  = static_cast<double>(-g[j]);
		s.atb_inf = std::max(s.atb_inf, std::fabs(s.atb[j]));
	}
	return s;
}

static double dot(const std::vector<double>& a, const std::vector<double>& b)
{
	double s = 0;
	for (size_t i = 0; i < a.size(); ++i) { s += a[i] * b[i]; }
	return s;
}

// The least-squares solution: Jacobi-preconditioned CG on the normal equations in double, restarted from the true residual
// (accumulated in long double) until that residual passes the certificate.  Exits 3 when it does not.
static std::vector<double> reference_solution(const fi::LinearEquation& eq, size_t n, const char* what)
{
	const Normal s = normal_of(eq, n);
	std::vector<double> x(n, 0.0), r = s.atb, z(n), p(n);
	bool certified = s.atb_inf == 0;
	for (size_t j = 0; j < n; ++j) {
		if (!(s.diag[j] > 0)) {
			std::printf("reference not converged: %s: unknown %zu has no equation\n", what, j);
			std::exit(3);
		}
	}
	long iterations = 0;
	double seen = 0;
	for (int outer = 0; outer < 60 && !certified; ++outer) {
		for (size_t j = 0; j < n; ++j) { p[j] = z[j] = r[j] / s.diag[j]; }
		double rz = dot(r, z);
		for (size_t it = 0; it < 20 * n + 100; ++it, ++iterations) {
			const std::vector<double> q = normal_product<double>(eq, p, false);
			const double pq = dot(p, q);
			if (!(pq > 0)) { break; }
			const double alpha = rz / pq;
			double rinf = 0;
			for (size_t j = 0; j < n; ++j) {
				x[j] += alpha * p[j];
				r[j] -= alpha * q[j];
				rinf = std::max(rinf, std::fabs(r[j]));
			}
			if (rinf <= 0.1e-12 * s.atb_inf) { break; }
			for (size_t j = 0; j < n; ++j) { z[j] = r[j] / s.diag[j]; }
			const double rz_new = dot(r, z), beta = rz_new / rz;
			rz = rz_new;
			for (size_t j = 0; j < n; ++j) { p[j] = z[j] + beta * p[j]; }
		}
		const std::vector<long double> g = normal_product<long double>(eq, x, true);
		seen = 0;
		for (size_t j = 0; j < n; ++j) {
			r[j] = static_cast<double>(-g[j]);
			seen = std::max(seen, std::fabs(r[j]));
		}
		certified = seen <= 1e-12 * s.atb_inf;
	}
	if (!certified) {
		std::printf("reference not converged: %s: |A^T(Ax-b)|_inf = %.3e, |A^T b|_inf = %.3e after %ld iterations\n", what, seen, s.atb_inf,
		            iterations);
		std::exit(3);
	}
	return x;
}

// k sweeps of x_j <- w (A^T b - R x)_j / D_j + (1 - w) x_j, R = A^T A - D, every sweep from the complete previous x: the
// update rule of the oracle's jacobi_iterations (oracle/fi_oracle.cpp, jacobi_sweeps), in double
static std::vector<double> reference_jacobi(const fi::LinearEquation& eq, const std::vector<float>& guess, int sweeps, double w)
{
	const size_t n = guess.size();
	const Normal s = normal_of(eq, n);
	std::vector<double> x(guess.begin(), guess.end());
	for (int k = 0; k < sweeps; ++k) {
		const std::vector<double> ax = normal_product<double>(eq, x, false);
		for (size_t j = 0; j < n; ++j) { x[j] = w * (s.atb[j] - (ax[j] - s.diag[j] * x[j])) / s.diag[j] + (1.0 - w) * x[j]; }
	}
	return x;
}

static double max_abs(const std::vector<double>& x)
{
	double m = 0;
	for (double v : x) { m = std::max(m, std::fabs(v)); }
	return m;
}

// max |got - want| / max |want|; +inf for a result of the wrong length (an empty vector is the library's "failed")
static double distance(const std::vector<float>& got, const std::vector<double>& want)
{
	if (got.size() != want.size()) { return INFINITY; }
	double num = 0;
	for (size_t i = 0; i < got.size(); ++i) {
		const double d = std::fabs(static_cast<double>(got[i]) - want[i]);
		num = std::max(num, d == d ? d : INFINITY);
	}
	return num / max_abs(want);
}

static double distance(const std::vector<double>& a, const std::vector<double>& b)
{
	double num = 0;
	for (size_t i = 0; i < a.size(); ++i) { num = std::max(num, std::fabs(a[i] - b[i])); }
	return num / max_abs(b);
}

static size_t unknowns(const std::vector<int>& sizes)
{
	size_t n = 1;
	for (int s : sizes) { n *= static_cast<size_t>(s); }
	return n;
}

// ---- the fields of B and C2 -------------------------------------------------------------------------------------------------

struct Cloud {
	std::vector<float> pos, nrm, weight;
	int count(int D) const { return static_cast<int>(pos.size()) / D; }
};

// `count` oriented points on `shells` concentric circles / spheres around the lattice's centre, all at least one cell inside
// the lattice (every point emits all of its rows); the normals point outwards on even shells and inwards on odd ones.
static Cloud shells_cloud(const std::vector<int>& sizes, int count, int shells, float reach, float dx, float dy)
{
	const int D = static_cast<int>(sizes.size());
	Cloud c;
	for (int i = 0; i < count; ++i) {
		const int   shell = i % shells;
		const float r = reach * (shell + 1) / shells, sign = shell % 2 ? -1.0f : 1.0f;
		const float a = 6.2831853f * ((i * 37) % count) / count, b = 3.1415927f * (0.08f + 0.84f * ((i * 101) % count) / count);
		const float dir[3] = {D == 2 ? std::cos(a) : std::sin(b) * std::cos(a), D == 2 ? std::sin(a) : std::sin(b) * std::sin(a), std::cos(b)};
		for (int d = 0; d < D; ++d) {
			c.pos.push_back(0.5f * (sizes[d] - 1) + r * dir[d] + 0.2f * std::sin(17.0f * i + 5.0f * d) + (d == 0 ? dx : d == 1 ? dy : 0.0f));
			c.nrm.push_back(sign * dir[d]);
		}
	}
	return c;
}

static fi::Weights rich_weights()  // three model terms: a model range of more than 2 x 4096 rows on these lattices
{
	fi::Weights w;
	w.model_0 = 0.05f;
	w.model_1 = 0.1f;
	w.model_2 = 0.5f;
	return w;
}

static fi::LatticeField field_2d()
{
	const std::vector<int> sizes{48, 40};
	const Cloud c = shells_cloud(sizes, 2800, 5, 17.5f, 0, 0);
	return fi::sdf_from_points(sizes, rich_weights(), c.count(2), c.pos.data(), c.nrm.data(), nullptr);
}

static fi::LatticeField field_3d()
{
	const std::vector<int> sizes{14, 12, 13};
	const Cloud c = shells_cloud(sizes, 2400, 2, 4.7f, 0, 0);
	fi::Weights w = rich_weights();
	w.model_2 = 0.0f;  // (two model terms are rows enough in 3-D, and the shortest gradient rows keep the sweep quick)
	w.gradient_kernel = fi::GradientKernel::kNearestNeighbor;
	return fi::sdf_from_points(sizes, w, c.count(3), c.pos.data(), c.nrm.data(), nullptr);
}

static fi::LatticeField field_by_hand()  // points, caller rows, model rows, more points (other kernels)
{
	const std::vector<int> sizes{48, 40};
	fi::LatticeField f{sizes};
	const Cloud a = shells_cloud(sizes, 2800, 5, 17.5f, 0, 0), b = shells_cloud(sizes, 2800, 4, 16.0f, 0.37f, -0.21f);
	fi::add_points(&f, 1.0f, fi::ValueKernel::kLinearInterpolation, 1.0f, fi::GradientKernel::kCellEdges, a.count(2), a.pos.data(),
	               a.nrm.data(), nullptr);
	for (int x = 0; x < 48; x += 5) { fi::add_equation(&f.eq, fi::Weight{0.1f}, fi::Rhs{2.0f}, {{x, 1.0f}, {39 * 48 + x, 0.5f}}); }
	fi::add_field_constraints(&f, rich_weights());
	fi::add_points(&f, 0.8f, fi::ValueKernel::kNearestNeighbor, 0.6f, fi::GradientKernel::kNearestNeighbor, b.count(2), b.pos.data(),
	               b.nrm.data(), nullptr);
	return f;
}

// the index rule of the sampled checksum this project used to have: of a range [a, b) it read a, a + step, ... and b - 1
static bool old_sampler_read(size_t i, size_t a, size_t b)
{
	const size_t n = b - a, step = n > 4096 ? n / 4096 : 1;
	return (i - a) % step == 0 || i == b - 1;
}

// ---- B. the note's validation, host only ------------------------------------------------------------------------------------

static bool valid(const fi::LatticeField& f) { return fi::detail::noted_rows_unchanged(f.eq, &f.sizes); }

static std::vector<size_t> swept(size_t a, size_t b)  // every 7th index of [a, b) plus the first and the last 64
{
	std::vector<size_t> idx;
	for (size_t i = a; i < b; ++i) {
		if ((i - a) % 7 == 0 || i - a < 64 || b - i <= 64) { idx.push_back(i); }
	}
	return idx;
}

static void sweep_field(const fi::LatticeField& original, const char* name, size_t expect_ranges)
{
	char msg[240];
	const size_t n = unknowns(original.sizes);
	require(original.eq.recipe && original.eq.recipe->segments.size() == expect_ranges, (std::string(name) + ": the expected noted ranges").c_str());
	require(valid(original), (std::string(name) + ": the untouched field is accepted").c_str());
	const std::vector<Segment>& segs = original.eq.recipe->segments;
	// The per-index edits are made in place and undone, which leaves what a fresh copy would hold (checked at the end); the
	// edits that move the vectors' contents work on real copies.
	fi::LatticeField f = original;
	require(valid(f), (std::string(name) + ": a copy of the field is accepted").c_str());
	long edits = 0, missed = 0;
	for (size_t k = 0; k < segs.size(); ++k) {
		const Segment& s = segs[k];
		std::snprintf(msg, sizeof msg, "%s: range %zu holds %zu triplets (>= 3 x 4096) and %zu rows (>= 2 x 4096), beyond the old sampler's reach", name, k,
		              s.trip1 - s.trip0, s.row1 - s.row0);
		require(s.trip1 - s.trip0 >= 3 * 4096 && s.row1 - s.row0 >= 2 * 4096, msg);
		long unread = 0;
		for (size_t i : swept(s.trip0, s.trip1)) {
			fi::Triplet& t = f.eq.triplets[i];
			const fi::Triplet keep = t;
			unread += !old_sampler_read(i, s.trip0, s.trip1);
			auto refused = [&](const char* edit) {
				++edits;
				if (valid(f)) {
					++missed;
					std::printf("   %s: range %zu, triplet %zu: %s was accepted\n", name, k, i, edit);
				}
				t = keep;
			};
			t.value = std::nextafterf(keep.value, 2.0f * std::fabs(keep.value) + 1.0f);
			refused("value -> nextafterf");
			if (keep.value != 0) {  // (0 x -40 is -0: no number changed, either answer is right)
				t.value = keep.value * -40.0f;
				refused("value x -40");
			}
			t.col = static_cast<size_t>(keep.col) + 1 < n ? keep.col + 1 : keep.col - 1;
			refused("col +- 1");
			t.row = static_cast<size_t>(keep.row) + 1 < s.row1 ? keep.row + 1 : keep.row - 1;
			refused("row -> a neighbouring noted row");
		}
		for (size_t i : swept(s.row0, s.row1)) {
			float& b = f.eq.rhs[i];
			const float keep = b;
			unread += !old_sampler_read(i, s.row0, s.row1);
			auto refused = [&](const char* edit) {
				++edits;
				if (valid(f)) {
					++missed;
					std::printf("   %s: range %zu, right-hand side %zu: %s was accepted\n", name, k, i, edit);
				}
				b = keep;
			};
			b = std::nextafterf(keep, 2.0f * std::fabs(keep) + 1.0f);
			refused("rhs -> nextafterf");
			b = keep + 1000.0f;
			refused("rhs += 1000");
		}
		std::snprintf(msg, sizeof msg, "%s: range %zu: the sweep visits indices the old sampler never read (%ld of them)", name, k, unread);
		require(unread > 1000, msg);
		const size_t tm = (s.trip0 + s.trip1) / 2, rm = (s.row0 + s.row1) / 2;
		auto structural = [&](const char* edit, const fi::LatticeField& g) {
			++edits;
			if (valid(g)) {
				++missed;
				std::printf("   %s: range %zu: %s was accepted\n", name, k, edit);
			}
		};
		{
			fi::LatticeField g = original;
			g.eq.triplets.erase(g.eq.triplets.begin() + static_cast<long>(tm));
			structural("erasing a triplet from the middle", g);
		}
		{
			fi::LatticeField g = original;
			const fi::Triplet& at = g.eq.triplets[tm];
			g.eq.triplets.insert(g.eq.triplets.begin() + static_cast<long>(tm), fi::Triplet(at.row, at.col, 0.125f));
			structural("inserting a triplet in the middle", g);
		}
		{
			fi::LatticeField g = original;
			g.eq.rhs.erase(g.eq.rhs.begin() + static_cast<long>(rm));
			structural("erasing a right-hand side", g);
		}
		{
			fi::LatticeField g = original;
			g.eq.rhs.insert(g.eq.rhs.begin() + static_cast<long>(rm), 3.25f);
			structural("inserting a right-hand side", g);
		}
	}
	{
		fi::LatticeField g = original;
		g.eq.triplets.resize(segs.back().trip1 - 1);
		++edits;
		if (valid(g)) {
			++missed;
			std::printf("   %s: triplets.resize(trip1 - 1) on the last range was accepted\n", name);
		}
		g = original;
		g.eq.rhs.assign(g.eq.rhs.size(), 0.0f);
		++edits;
		if (valid(g)) {
			++missed;
			std::printf("   %s: a right-hand side of zeros was accepted\n", name);
		}
	}
	std::snprintf(msg, sizeof msg, "%s: %ld edits of noted rows, every one refused (%ld accepted)", name, edits, missed);
	require(missed == 0, msg);
	const bool same = f.eq.rhs == original.eq.rhs && f.eq.triplets.size() == original.eq.triplets.size() &&
	                  std::memcmp(f.eq.triplets.data(), original.eq.triplets.data(), f.eq.triplets.size() * sizeof(fi::Triplet)) == 0;
	require(same && valid(f), (std::string(name) + ": every edit was undone: the field is the original again, and accepted").c_str());
	fi::LatticeField h = original;
	for (int x = 0; x < original.sizes[0]; x += 3) { fi::add_equation(&h.eq, fi::Weight{0.05f}, fi::Rhs{1.5f}, {{x, 1.0f}, {x + 1, -0.5f}}); }
	require(h.eq.rhs.size() > original.eq.rhs.size() && valid(h), (std::string(name) + ": rows appended with add_equation keep the note").c_str());
}

static int run_host(const std::string& which)
{
	if (which == "3d") { sweep_field(field_3d(), "3-D {14,12,13}", 2); }
	if (which == "hand") { sweep_field(field_by_hand(), "by hand (points, caller rows, model, points)", 3); }
	if (which != "2d") {
		std::printf("all host checks passed\n");
		return 0;
	}
	const fi::LatticeField f2 = field_2d();
	sweep_field(f2, "2-D {48,40}", 2);
	{
		size_t bytes = 0;
		for (const Segment& s : f2.eq.recipe->segments) { bytes += (s.trip1 - s.trip0) * sizeof(fi::Triplet) + (s.row1 - s.row0) * sizeof(float); }
		const int reps = 200;
		int accepted = 0;
		const auto t0 = std::chrono::steady_clock::now();
		for (int r = 0; r < reps; ++r) { accepted += valid(f2); }
		const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		const double gbs = 1e-9 * static_cast<double>(bytes) * reps / sec;
		std::printf("   validator throughput over the 2-D field: %.2f GB/s (%zu bytes per call, %.1f us); ESTIMATE for 1.2 GB of noted rows "
		            "(10^8 triplets): %.2f s per solve\n", gbs, bytes, 1e6 * sec / reps, 1.2 / gbs);
		require(accepted == reps, "the validator's answer does not change between calls");
	}
	std::printf("all host checks passed\n");
	return 0;
}

// ---- C2. edits the old sampler did not read -----------------------------------------------------------------------------------

struct Edit {
	std::string what;
	fi::LinearEquation eq;            // the edited system
	std::vector<double> solution;     // its reference solution
};

// Six edits per field -- two in the model range's triplets, two in a point range's triplets, two right-hand sides -- at
// indices old_sampler_read() is false for, each checked on the host alone to move the reference solution by at least
// 100 x `tolerance` (relative to max |x*|, like the comparisons that follow).
static std::vector<Edit> sized_edits(const fi::LatticeField& f, const char* name, double tolerance)
{
	const size_t n = unknowns(f.sizes);
	const std::vector<double> x0 = reference_solution(f.eq, n, name);
	const Segment *model = nullptr, *points = nullptr;
	for (const Segment& s : f.eq.recipe->segments) { (s.kind == Segment::kModel ? model : points) = &s; }
	require(model && points, (std::string(name) + ": a model range and a point range").c_str());
	std::vector<Edit> edits;
	char what[200];
	// a coefficient x -40: where the row's term value * x*[col] is largest (the edit's pull grows with it), and once more in
	// another row, at least 100 triplets away
	for (const Segment* s : {model, points}) {
		size_t first = 0;
		for (int pick = 0; pick < 2; ++pick) {
			size_t best = 0;
			double term = -1;
			for (size_t i = s->trip0; i < s->trip1; ++i) {
				const fi::Triplet& t = f.eq.triplets[i];
				const double v = std::fabs(t.value * x0[static_cast<size_t>(t.col)]);
				const bool far = pick == 0 || (i > first ? i - first : first - i) >= 100;
				if (!old_sampler_read(i, s->trip0, s->trip1) && far && v > term) {
					term = v;
					best = i;
				}
			}
			first = best;
			Edit e;
			e.eq = f.eq;
			e.eq.triplets[best].value *= -40.0f;
			std::snprintf(what, sizeof what, "%s: %s triplet %zu (+%zu in its range), value x -40", name, s == model ? "model" : "point", best,
			              best - s->trip0);
			e.what = what;
			edits.push_back(e);
		}
	}
	for (const Segment* s : {model, points}) {
		size_t row = s->row0 + (s->row1 - s->row0) / 3;
		while (old_sampler_read(row, s->row0, s->row1)) { ++row; }
		Edit e;
		e.eq = f.eq;
		e.eq.rhs[row] += 1000.0f;
		std::snprintf(what, sizeof what, "%s: %s right-hand side %zu (+%zu in its range) += 1000", name, s == model ? "model" : "point", row, row - s->row0);
		e.what = what;
		edits.push_back(e);
	}
	for (Edit& e : edits) {
		e.solution = reference_solution(e.eq, n, e.what.c_str());
		double moved = 0;
		for (size_t j = 0; j < n; ++j) { moved = std::max(moved, std::fabs(e.solution[j] - x0[j])); }
		const double scale = std::max(max_abs(e.solution), max_abs(x0));
		std::printf("   %s: the reference moves by %.3e = %.0f x tolerance (max |x*| %.3f)\n", e.what.c_str(), moved, moved / (tolerance * scale), scale);
		require(moved >= 100 * tolerance * scale, (e.what + ": moves the reference solution by >= 100 x tolerance").c_str());
	}
	return edits;
}

static const double kTolExact = 1e-5;   // BASELINE's tolerance for fp64 solves (tests/test_gpu_solve.py)
static const double kTolJacobi = 2e-5;  // the project's figure for 25-odd fp32 sweeps against a reference
static const double kTolCg32 = 5e-4;    // fp32 CG to a 1e-7 residual at this size (tests/cxx/test_dropin.cpp 6(a))

static fi::SolveOptions cg_options(bool tile)
{
	fi::SolveOptions o;
	o.tile = tile;
	o.tile_size = 8;
	o.error_tolerance = 1e-7f;
	o.max_iterations = 20000;
	return o;
}

static int run_c2(bool device)
{
	char msg[320];
	const fi::LatticeField fields[2] = {field_2d(), field_3d()};
	const char* names[2] = {"2-D {48,40}", "3-D {14,12,13}"};
	for (int k = 0; k < 2; ++k) {
		const fi::LatticeField& f = fields[k];
		const size_t n = unknowns(f.sizes);
		const std::vector<Edit> edits = sized_edits(f, names[k], kTolCg32);  // (the larger of the two tolerances used below)
		if (!device) { continue; }
		const std::vector<float> zero(n, 0.0f);
		for (const Edit& e : edits) {
			const std::vector<float> exact = fi::solve_sparse_linear_exact(e.eq, static_cast<int>(n));
			const bool mf1 = fi::last_solve_was_matrix_free();
			const std::vector<float> cg = fi::solve_tiled_with_guess(e.eq, zero, f.sizes, cg_options(false));
			const bool mf2 = fi::last_solve_was_matrix_free();
			const double d1 = distance(exact, e.solution), d2 = distance(cg, e.solution);
			std::snprintf(msg, sizeof msg, "%s: the edited rows are solved: exact %.2e (<= %.0e)%s, solve_tiled_with_guess %.2e (<= %.0e)%s", e.what.c_str(),
			              d1, kTolExact, mf1 ? " MATRIX-FREE" : "", d2, kTolCg32, mf2 ? " MATRIX-FREE" : "");
			require(d1 <= kTolExact && d2 <= kTolCg32, msg);
		}
	}
	std::printf(device ? "all c2 checks passed\n" : "all sizing checks passed\n");
	return 0;
}

// ---- C1. rows re-made from the note == the rows in eq -------------------------------------------------------------------------

// A cloud for `sizes` with, beside `ordinary` points on a circle / sphere, points whose coordinates sit where the host row
// builders and the device assembly must make the same choice: in the shells [-1, 0) and [size-1, size), exactly 0 and
// size-1, exact integers, the rounding ties x.5, and more than one cell outside.  weight: every fifth point exactly 0.
static Cloud edge_cloud(const std::vector<int>& sizes, int ordinary)
{
	const int D = static_cast<int>(sizes.size());
	Cloud c = shells_cloud(sizes, ordinary, 1, 0.3f * (*std::min_element(sizes.begin(), sizes.end()) - 1), 0, 0);
	if (D == 1) {  // (a "circle" in 1-D is two points: spread the ordinary points over the line instead)
		for (int i = 0; i < ordinary; ++i) {
			c.pos[static_cast<size_t>(i)] = 1.3f + std::fmod(7.77f * i, sizes[0] - 3.0f);
			c.nrm[static_cast<size_t>(i)] = i % 3 ? 1.0f : -1.0f;
		}
	}
	auto special = [&](int d, int k) -> float {
		const float s = static_cast<float>(sizes[d]);
		const float at[] = {-1.0f, -0.5f, -0.001f, -0.4f, 0.0f, 1.0f, 5.0f, s - 1.0f, s - 0.5f, s - 0.25f, s - 0.6f, s - 2.0f, 2.5f, 0.5f, s - 2.5f,
		                    s - 1.5f, -1.75f, s + 0.8f, -3.2f, s, -1.001f, s - 1.001f};
		return at[static_cast<size_t>(k) % (sizeof at / sizeof at[0])];
	};
	const int kinds = 22;
	int serial = 0;
	auto push = [&](const float* p) {
		float nn = 0, g[3];
		for (int d = 0; d < D; ++d) {
			g[d] = std::sin(1.7f * serial + 2.1f * d + 0.3f);
			nn += g[d] * g[d];
		}
		for (int d = 0; d < D; ++d) {
			c.pos.push_back(p[d]);
			c.nrm.push_back(g[d] / std::sqrt(nn));
		}
		++serial;
	};
	for (int k = 0; k < kinds; ++k) {
		for (int axis = 0; axis < D; ++axis) {  // special along one axis, inside along the others (integers and fractions)
			float p[3];
			for (int d = 0; d < D; ++d) { p[d] = d == axis ? special(d, k) : 2.0f + static_cast<float>((3 * k + 5 * d) % (sizes[d] - 4)) + (k % 2 ? 0.37f : 0.0f); }
			push(p);
		}
		if (D > 1) {  // special along every axis
			float p[3];
			for (int d = 0; d < D; ++d) { p[d] = special(d, k + 3 * d); }
			push(p);
			for (int d = 0; d < D; ++d) { p[d] = special(d, k + (d ? 7 : 0)); }
			push(p);
		}
	}
	const int count = c.count(D);
	for (int i = 0; i < count; ++i) { c.weight.push_back(i % 5 == 0 ? 0.0f : 0.5f + 0.25f * static_cast<float>(i % 3)); }
	return c;
}

struct Case {
	const char* name;
	fi::Weights weights;  // with its kernels
	bool point_weights;   // the array with exact zeros; else null
	bool extra_rows;      // rows of the caller's own after the noted ones
	bool plain;           // default weights and kernels: the matrix-free path must be taken
};

static std::vector<Case> cases()
{
	using V = fi::ValueKernel;
	using G = fi::GradientKernel;
	auto with = [](fi::Weights w, V v, G g) {
		w.value_kernel = v;
		w.gradient_kernel = g;
		return w;
	};
	fi::Weights w0;          // default: model_2 alone
	fi::Weights w1;          // model_0 + model_1 only
	w1.model_0 = 0.05f;
	w1.model_1 = 0.4f;
	w1.model_2 = 0.0f;
	fi::Weights w2;          // the higher orders and the gradient smoothness (model_0 bounds the condition number: fp32 CG follows)
	w2.model_0 = 0.1f;
	w2.model_1 = 0.2f;
	w2.model_2 = 0.3f;
	w2.model_3 = 0.1f;
	w2.model_4 = 0.05f;
	w2.gradient_smoothness = 0.2f;
	fi::Weights w3 = w0;     // a term set to 0: no value rows at all
	w3.data_pos = 0.0f;
	w3.model_0 = 0.05f;
	fi::Weights w4 = w0;     // a term set to 0: no gradient rows at all
	w4.data_gradient = 0.0f;
	// every value kernel with every gradient kernel, every weight set with and without point weights or in two kernel pairs
	return {
	    {"default weights, linear / cell edges, no point weights", with(w0, V::kLinearInterpolation, G::kCellEdges), false, true, true},
	    {"default weights, nearest / nearest, point weights with zeros", with(w0, V::kNearestNeighbor, G::kNearestNeighbor), true, false, false},
	    {"model_0 + model_1, linear / linear, point weights with zeros", with(w1, V::kLinearInterpolation, G::kLinearInterpolation), true, true, false},
	    {"model_0 + model_1, nearest / cell edges, no point weights", with(w1, V::kNearestNeighbor, G::kCellEdges), false, false, false},
	    {"model_0..4 + gradient smoothness, linear / nearest, no point weights", with(w2, V::kLinearInterpolation, G::kNearestNeighbor), false, false, false},
	    {"model_0..4 + gradient smoothness, nearest / linear, point weights with zeros", with(w2, V::kNearestNeighbor, G::kLinearInterpolation), true, true, false},
	    {"data_pos = 0, linear / cell edges, point weights with zeros", with(w3, V::kLinearInterpolation, G::kCellEdges), true, false, false},
	    {"data_gradient = 0, nearest / linear, no point weights", with(w4, V::kNearestNeighbor, G::kLinearInterpolation), false, true, false},
	};
}

static int run_c1(int D, bool device)
{
	const std::vector<int> sizes = D == 1 ? std::vector<int>{96} : D == 2 ? std::vector<int>{48, 40} : std::vector<int>{14, 12, 13};
	const size_t n = unknowns(sizes);
	const Cloud cloud = edge_cloud(sizes, D == 1 ? 40 : D == 2 ? 300 : 400);
	char msg[400];
	std::vector<float> guess(n), zero(n, 0.0f);
	for (size_t i = 0; i < n; ++i) { guess[i] = std::sin(0.37f * static_cast<float>(i)); }
	for (const Case& c : cases()) {
		fi::LatticeField f = fi::sdf_from_points(sizes, c.weights, cloud.count(D), cloud.pos.data(), cloud.nrm.data(),
		                                         c.point_weights ? cloud.weight.data() : nullptr);
		if (c.extra_rows) {
			for (size_t j = 0; j < n; j += 11) { fi::add_equation(&f.eq, fi::Weight{0.05f}, fi::Rhs{1.0f + 0.01f * static_cast<float>(j % 50)}, {{static_cast<int>(j), 1.0f}}); }
		}
		std::snprintf(msg, sizeof msg, "%d-D, %s", D, c.name);
		const std::string name = msg;
		const std::vector<double> x = reference_solution(f.eq, n, name.c_str());
		const std::vector<double> jac = reference_jacobi(f.eq, guess, 25, 0.5);
		std::printf("   %s: %zu rows, %zu triplets, max |x*| %.3f; reference certified\n", name.c_str(), f.eq.rhs.size(), f.eq.triplets.size(), max_abs(x));
		require(max_abs(x) > 1e-3 && fi::detail::noted_rows_unchanged(f.eq, &sizes), (name + ": a field to compare, its note valid").c_str());
		if (!device) { continue; }
		keep_going = true;
		bool all_mf = true;
		auto mf = [&] { all_mf = all_mf && fi::last_solve_was_matrix_free(); };
		const double d_exact = distance(fi::solve_sparse_linear_exact(f.eq, static_cast<int>(n)), x);
		mf();
		const double d_jac = distance(fi::jacobi_iterations(f.eq, guess, 25, 0.5f), jac);
		mf();
		const double d_fast = distance(fi::solve_sparse_linear_fast(f.eq, static_cast<int>(n)), x);
		mf();
		const double d_guess = distance(fi::solve_sparse_linear_with_guess(f.eq, zero, 20000, 1e-7f), x);
		mf();
		const double d_tile = distance(fi::solve_tiled_with_guess(f.eq, zero, sizes, cg_options(true)), x);
		mf();
		const double d_cg = distance(fi::solve_tiled_with_guess(f.eq, zero, sizes, cg_options(false)), x);
		mf();
		std::printf("   %s: exact %.2e, jacobi %.2e, fast %.2e, with_guess %.2e, tiled(tile) %.2e, tiled(no tile) %.2e%s\n", name.c_str(), d_exact, d_jac,
		            d_fast, d_guess, d_tile, d_cg, all_mf ? "; all matrix-free" : "");
		require(d_exact <= kTolExact, (name + ": solve_sparse_linear_exact == reference to 1e-5").c_str());
		require(d_jac <= kTolJacobi, (name + ": jacobi_iterations(25, 0.5) == 25 reference sweeps to 2e-5").c_str());
		require(d_fast <= kTolCg32 && d_guess <= kTolCg32 && d_tile <= kTolCg32 && d_cg <= kTolCg32,
		        (name + ": fast, with_guess, tiled (tile on / off) == reference to 5e-4").c_str());
		if (c.plain) { require(all_mf, (name + ": every one of these calls ran matrix-free").c_str()); }
	}
	if (failures) {
		std::printf("%d c1 checks FAILED\n", failures);
		return 1;
	}
	std::printf(device ? "all c1 checks passed\n" : "all c1 references certified\n");
	return 0;
}

// ---- C3. one cached context, several systems -----------------------------------------------------------------------------------

static int run_c3()
{
	const std::vector<int> sizes{48, 40};
	const size_t n = unknowns(sizes);
	const std::vector<float> zero(n, 0.0f);
	const Cloud ca = edge_cloud(sizes, 300), cb = shells_cloud(sizes, 120, 2, 12.0f, 0, 0);
	fi::LatticeField a = fi::sdf_from_points(sizes, fi::Weights{}, ca.count(2), ca.pos.data(), ca.nrm.data(), nullptr);
	for (size_t j = 0; j < n; j += 11) { fi::add_equation(&a.eq, fi::Weight{0.05f}, fi::Rhs{1.0f}, {{static_cast<int>(j), 1.0f}}); }
	fi::Weights wb;
	wb.model_1 = 0.3f;
	wb.model_2 = 0.2f;
	wb.data_gradient = 0.5f;
	const fi::LatticeField b = fi::sdf_from_points(sizes, wb, cb.count(2), cb.pos.data(), cb.nrm.data(), nullptr);
	const std::vector<double> xa = reference_solution(a.eq, n, "c3: field A"), xb = reference_solution(b.eq, n, "c3: field B");
	require(distance(xa, xb) > 0.1, "c3: A and B are different fields");
	const fi::SolveOptions o = cg_options(false);
	const std::vector<float> a1 = fi::solve_tiled_with_guess(a.eq, zero, sizes, o);
	require(fi::last_solve_was_matrix_free() && distance(a1, xa) <= kTolCg32, "c3: 1. A, matrix-free == reference");
	const std::vector<float> b2 = fi::solve_tiled_with_guess(b.eq, zero, sizes, o);
	require(fi::last_solve_was_matrix_free() && distance(b2, xb) <= kTolCg32, "c3: 2. B (other weights, fewer points, no extra rows), matrix-free == reference");
	const std::vector<float> a3 = fi::solve_tiled_with_guess(a.eq, zero, sizes, o);
	require(fi::last_solve_was_matrix_free() && distance(a3, xa) <= kTolCg32, "c3: 3. A again, matrix-free == reference");
	setenv("FI_DROPIN_NO_RECIPE", "1", 1);
	const std::vector<float> a4 = fi::solve_tiled_with_guess(a.eq, zero, sizes, o);
	unsetenv("FI_DROPIN_NO_RECIPE");
	std::printf("   generic rows of A in the context B and A just used: %.2e from the reference\n", distance(a4, xa));
	require(!fi::last_solve_was_matrix_free() && distance(a4, xa) <= kTolCg32, "c3: 4. A through the generic rows == reference");
	const std::vector<float> a5 = fi::solve_tiled_with_guess(a.eq, zero, sizes, o);
	require(fi::last_solve_was_matrix_free() && a5.size() == n, "c3: 5. A again, matrix-free");
	const bool same = a1.size() == n && a3.size() == n && std::memcmp(a1.data(), a3.data(), n * sizeof(float)) == 0 &&
	                  std::memcmp(a1.data(), a5.data(), n * sizeof(float)) == 0;
	require(same, "c3: the three matrix-free solves of A return the same bits");
	std::printf("all c3 checks passed\n");
	return 0;
}

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	const std::string which = argc > 2 ? argv[2] : "";
	const int D = std::atoi(which.c_str());
	const bool dry = argc > 3 && std::string(argv[3]) == "references";  // c1's host half alone
	if (mode == "host" && (which == "2d" || which == "3d" || which == "hand")) { return run_host(which); }
	if (mode == "sizing") { return run_c2(false); }
	if (mode == "c1" && D >= 1 && D <= 3) { return run_c1(D, !dry); }
	if (mode == "c2") { return run_c2(true); }
	if (mode == "c3") { return run_c3(); }
	std::printf("usage: test_recipe host <2d|3d|hand> | sizing | c1 <1|2|3> [references] | c2 | c3\n");
	return 2;
}
