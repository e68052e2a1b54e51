// test_transfer.hip -- every grid-transfer kernel of field_interpolation_amd/csrc/fi_transfer.hip against a reference of the
// same operation, path by path.  The three launchers (fi::launch_prolong, fi::launch_prolong_cubic, fi::launch_restrict) are
// called directly with hand-filled fi::LevelPair's; no solve is involved.
//
// The reference is written from the GEOMETRY of the two lattices, not from the kernels' tap functions: a dense matrix per
// axis (nf x nc) whose rows are Lagrange weights, computed as integer fractions, of the coarse nodes a fine point draws on
//   vertex-centred axis: nc = (nf+1)/2, coarse node j at fine coordinate 2j
//   cell-centred axis (even nf): nc = nf/2, coarse node j at fine coordinate 2j + 1/2
// R is the transpose of the linear P; 2-D / 3-D operators are tensor products, applied separably in fp64.
//
// On integer inputs in [-1000, 1000] every product and partial sum of P x, fine + P x and P^T y is a multiple of 1/64 below
// 2^18: any order of summation is exact in fp32 and fp64, so the device must return the reference's bits (the `host`
// group asserts the premise 64 max sum |w x| < 2^24 from the reference alone).  Everything else is held to
// |got - ref| <= k u sum |w||x| with k the longest chain of roundings.  Outputs are pre-filled with a NaN pattern: what a
// kernel does not own must keep it.
//
// usage: test_transfer host | prolong | cubic | restrict | slabs      (`host` makes no HIP call)
#include "fi_solver_internal.h"

#include <cstdio>

namespace {

typedef std::vector<double> Vd;

[[noreturn]] void die(const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	std::vprintf(fmt, ap);
	va_end(ap);
	std::printf("\n");
	std::fflush(stdout);
	std::_Exit(1);
}
#define REQUIRE(cond, ...) do { if (!(cond)) { std::printf("FAILED %s (line %d): ", #cond, __LINE__); die(__VA_ARGS__); } } while (0)
// the first HIP error ends the program: nothing is launched after it
#define HIP_OK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { std::printf("HIP error: %s -> %s\n", #call, hipGetErrorString(e_)); std::fflush(stdout); std::_Exit(3); } } while (0)

// ---- the reference: one dense matrix per axis, from the geometry ------------------------------------------------

long long gcd_ll(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a < 0 ? -a : a; }

// coordinates in units of half a fine spacing, so that all are integers: fine f at 2f, coarse j at 4j (vertex) / 4j + 1 (cell)
int fine_x(int f) { return 2 * f; }
int coarse_x(int j, int cc) { return cc ? 4 * j + 1 : 4 * j; }

// weight of node k of the Lagrange polynomial through `cnt` coarse nodes at fine point f, as an exact dyadic fraction
double lagrange(const int* nodes, int cnt, int k, int cc, int f)
{
	long long num = 1, den = 1;
	for (int m = 0; m < cnt; ++m) {
		if (m == k) { continue; }
		num *= fine_x(f) - coarse_x(nodes[m], cc);
		den *= coarse_x(nodes[k], cc) - coarse_x(nodes[m], cc);
	}
	if (den < 0) { num = -num; den = -den; }
	const long long g = gcd_ll(num, den);
	num /= g;
	den /= g;
	REQUIRE((den & (den - 1)) == 0, "weight %lld/%lld is not dyadic", num, den);
	return static_cast<double>(num) / static_cast<double>(den);  // (exact)
}

struct AxisRef {
	int nf = 1, nc = 1, cc = 0;
	Vd lin, cub;                // nf x nc, row major
	std::vector<char> copied;   // linear row: the copied last point of an even vertex-centred extent
	std::vector<char> four;     // cubic row: four taps
};

void lagrange_row(Vd& M, int nc, int cc, int f, int first, int cnt)
{
	int nodes[4];
	for (int k = 0; k < cnt; ++k) { nodes[k] = first + k; }
	for (int k = 0; k < cnt; ++k) { M[static_cast<size_t>(f) * nc + nodes[k]] += lagrange(nodes, cnt, k, cc, f); }
}

AxisRef make_axis(int nf, int cc)
{
	REQUIRE(!cc || nf % 2 == 0, "a cell-centred axis has an even extent (%d)", nf);
	AxisRef A;
	A.nf = nf;
	A.nc = (nf + 1) / 2;
	A.cc = cc;
	const int nc = A.nc;
	A.lin.assign(static_cast<size_t>(nf) * nc, 0.0);
	A.cub.assign(static_cast<size_t>(nf) * nc, 0.0);
	A.copied.assign(nf, 0);
	A.four.assign(nf, 0);
	for (int f = 0; f < nf; ++f) {
		const int j = f >> 1;
		double* lin = &A.lin[static_cast<size_t>(f) * nc];
		if (!cc) {
			if (!(f & 1)) { lin[j] = 1.0; }                             // fine 2i IS coarse i
			else if (j + 1 < nc) { lagrange_row(A.lin, nc, 0, f, j, 2); }  // the mean of its two neighbours
			else { lin[j] = 1.0; A.copied[f] = 1; }                     // even extent: the last point copies its only neighbour
		} else {
			const int nb = (f & 1) ? j + 1 : j - 1;  // the next coarse node on f's side
			if (nb >= 0 && nb < nc) { lagrange_row(A.lin, nc, 1, f, nb < j ? nb : j, 2); }
			else { lagrange_row(A.lin, nc, 1, f, (f & 1) ? j - 1 : j, 2); }  // extrapolated through the two nearest nodes
		}
		bool four = false;
		int  base = 0;
		if (!cc) {
			if (!(f & 1)) { A.cub[static_cast<size_t>(f) * nc + j] = 1.0; continue; }
			four = j >= 1 && j + 2 <= nc - 1;
			base = j - 1;
		} else {
			base = (f & 1) ? j - 1 : j - 2;
			four = base >= 0 && base + 3 < nc;
		}
		if (four) {
			lagrange_row(A.cub, nc, cc, f, base, 4);
			A.four[f] = 1;
		} else {
			for (int k = 0; k < nc; ++k) { A.cub[static_cast<size_t>(f) * nc + k] = lin[k]; }
		}
	}
	return A;
}

// what the reference must satisfy on its own, per extent and halving
void check_axis(const AxisRef& A)
{
	const int nf = A.nf, nc = A.nc, cc = A.cc;
	for (int f = 0; f < nf; ++f) {
		double sl = 0, sc = 0, linv = 0, cubv = 0;
		auto poly = [](double x) { return 3.0 - 2.0 * x + 5.0 * x * x - x * x * x; };  // (integers: exact in fp64)
		for (int k = 0; k < nc; ++k) {
			const double wl = A.lin[static_cast<size_t>(f) * nc + k], wc = A.cub[static_cast<size_t>(f) * nc + k];
			sl += wl;
			sc += wc;
			linv += wl * (7.0 + 3.0 * coarse_x(k, cc));
			cubv += wc * poly(coarse_x(k, cc));
		}
		REQUIRE(sl == 1.0 && sc == 1.0, "nf %d cc %d: row %d sums to %g (linear), %g (cubic)", nf, cc, f, sl, sc);
		if (!A.copied[f]) { REQUIRE(linv == 7.0 + 3.0 * fine_x(f), "nf %d cc %d: linear P loses a linear function at %d", nf, cc, f); }
		if (A.four[f]) { REQUIRE(cubv == poly(fine_x(f)), "nf %d cc %d: cubic P loses a cubic at %d: %g", nf, cc, f, cubv); }
		else if (!A.copied[f]) {
			double v = 0;
			for (int k = 0; k < nc; ++k) { v += A.cub[static_cast<size_t>(f) * nc + k] * (7.0 + 3.0 * coarse_x(k, cc)); }
			REQUIRE(v == 7.0 + 3.0 * fine_x(f), "nf %d cc %d: cubic P loses a linear function at %d", nf, cc, f);
		}
	}
	// the documented interior rows
	const int f = 9, j = 4;  // odd, four taps fit for every extent >= 15
	const double* row = &A.cub[static_cast<size_t>(f) * nc];
	if (cc) {
		REQUIRE(row[j - 1] == -14.0 / 256 && row[j] == 210.0 / 256 && row[j + 1] == 70.0 / 256 && row[j + 2] == -10.0 / 256,
		        "nf %d: cell-centred cubic row %g %g %g %g", nf, row[j - 1], row[j], row[j + 1], row[j + 2]);
		const double* ev = &A.cub[static_cast<size_t>(f - 1) * nc];
		REQUIRE(ev[j - 2] == -10.0 / 256 && ev[j - 1] == 70.0 / 256 && ev[j] == 210.0 / 256 && ev[j + 1] == -14.0 / 256, "nf %d: mirrored row", nf);
		REQUIRE(A.lin[0] == 1.25 && A.lin[1] == -0.25 && A.lin[static_cast<size_t>(2) * nc + 1] == 0.75 && A.lin[static_cast<size_t>(2) * nc] == 0.25,
		        "nf %d: cell-centred linear rows", nf);
	} else {
		REQUIRE(row[j - 1] == -1.0 / 16 && row[j] == 9.0 / 16 && row[j + 1] == 9.0 / 16 && row[j + 2] == -1.0 / 16, "nf %d: vertex-centred cubic row", nf);
		REQUIRE(A.lin[static_cast<size_t>(f) * nc + j] == 0.5 && A.lin[static_cast<size_t>(f) * nc + j + 1] == 0.5, "nf %d: vertex-centred linear row", nf);
	}
}

// a per-axis operator in compressed rows (of the dense matrix or of its transpose)
struct Sp {
	int nout = 1, nin = 1;
	std::vector<int> ptr{0, 1}, idx{0};
	Vd w{1.0};
};
Sp sparse(const Vd& M, int nf, int nc, bool transpose)
{
	Sp s;
	s.nout = transpose ? nc : nf;
	s.nin  = transpose ? nf : nc;
	s.ptr.assign(1, 0);
	s.idx.clear();
	s.w.clear();
	for (int o = 0; o < s.nout; ++o) {
		for (int i = 0; i < s.nin; ++i) {
			const double v = transpose ? M[static_cast<size_t>(i) * nc + o] : M[static_cast<size_t>(o) * nc + i];
			if (v != 0.0) { s.idx.push_back(i); s.w.push_back(v); }
		}
		s.ptr.push_back(static_cast<int>(s.idx.size()));
	}
	return s;
}
// out = op applied along axis d of `in` (extents din, x fastest); absw: |w| (for sum |w||x| on |x|)
Vd apply_axis(const Sp& op, int d, const int* din, const Vd& in, bool absw)
{
	size_t inner = 1, outer = 1;
	for (int e = 0; e < d; ++e) { inner *= din[e]; }
	for (int e = d + 1; e < 3; ++e) { outer *= din[e]; }
	REQUIRE(din[d] == op.nin && in.size() == inner * outer * op.nin, "apply_axis: extents");
	Vd out(inner * outer * op.nout, 0.0);
	for (size_t o = 0; o < outer; ++o) {
		for (int i = 0; i < op.nout; ++i) {
			double* dst = &out[(o * op.nout + i) * inner];
			for (int t = op.ptr[i]; t < op.ptr[i + 1]; ++t) {
				const double  w   = absw ? std::fabs(op.w[t]) : op.w[t];
				const double* src = &in[(o * op.nin + op.idx[t]) * inner];
				for (size_t s = 0; s < inner; ++s) { dst[s] += w * src[s]; }
			}
		}
	}
	return out;
}
Vd apply3(const Sp* ops, const int* din, const Vd& in, bool absw)
{
	int dims[3] = {din[0], din[1], din[2]};
	Vd v = in;
	for (int d = 0; d < 3; ++d) {
		v = apply_axis(ops[d], d, dims, v, absw);
		dims[d] = ops[d].nout;
	}
	return v;
}

// ---- cases ------------------------------------------------------------------------------------------------------

enum Op { PROLONG, CUBIC, RESTRICT };
// inputs: integers in [-1000, 1000]; normal deviates rounded to fp32 (what an fp32 kernel is given); normal deviates in fp64
enum Kind { INT, REAL32, REAL64 };
const char* const kSwitches[] = {"FI_BLOCK_PROLONG", "FI_FLAT_RESTRICT", "FI_ONE_PASS_RESTRICT", "FI_TILED_RESTRICT"};

struct Case {
	Op  op;
	int ndim;
	int nf[3];
	int cc[3];
	const char* sw;  // a test switch set around the launch, or nullptr
	bool two_pass;   // restriction: a work array is given
	int  ranks;      // 1: undivided
	int nc(int d) const { return (nf[d] + 1) / 2; }
};

Case make_case(Op op, std::vector<int> nf, std::vector<int> cc, const char* sw = nullptr, bool two_pass = false, int ranks = 1)
{
	Case c{};
	c.op = op;
	c.ndim = static_cast<int>(nf.size());
	for (int d = 0; d < 3; ++d) {
		c.nf[d] = d < c.ndim ? nf[d] : 1;
		c.cc[d] = d < c.ndim ? cc[d] : 0;
	}
	c.sw = sw;
	c.two_pass = two_pass;
	c.ranks = ranks;
	return c;
}
std::vector<int> halved(const std::vector<int>& nf)  // the hierarchy's own choice: even extents cell-centred
{
	std::vector<int> cc;
	for (int n : nf) { cc.push_back(n % 2 == 0); }
	return cc;
}
// the halvings of a small shape: the default, every axis vertex-centred (FI_VERTEX_LEVELS), and only the slowest axis
// vertex-centred (a slab level whose stencils reach one plane)
std::vector<std::vector<int>> halvings(const std::vector<int>& nf)
{
	std::vector<std::vector<int>> out{halved(nf)};
	std::vector<int> vertex(nf.size(), 0), last = out[0];
	last.back() = 0;
	if (vertex != out[0]) { out.push_back(vertex); }
	if (last != out[0] && last != vertex) { out.push_back(last); }
	return out;
}

std::vector<Case> cases_of(const std::string& group)
{
	typedef std::vector<int> S;
	std::vector<Case> v;
	auto small = [&](Op op, S nf, bool two_pass = false) {
		for (const auto& cc : halvings(nf)) { v.push_back(make_case(op, nf, cc, nullptr, two_pass)); }
	};
	if (group == "prolong") {
		for (S nf : {S{17}, S{16}, S{30}}) { small(PROLONG, nf); }
		for (S nf : {S{17, 16}, S{16, 18}, S{33, 19}, S{30, 22}}) { small(PROLONG, nf); }
		for (S nf : {S{17, 16, 19}, S{16, 16, 16}, S{21, 18, 16}}) { small(PROLONG, nf); }
		for (S nf : {S{256, 128, 128}, S{264, 132, 130}}) {
			v.push_back(make_case(PROLONG, nf, halved(nf)));
			v.push_back(make_case(PROLONG, nf, halved(nf), "FI_BLOCK_PROLONG"));
		}
	} else if (group == "cubic") {
		for (S nf : {S{17, 16, 19}, S{16, 16, 16}, S{31, 22, 17}}) { small(CUBIC, nf); }
		for (S nf : {S{256, 128, 128}, S{264, 132, 130}}) {
			v.push_back(make_case(CUBIC, nf, halved(nf)));
			v.push_back(make_case(CUBIC, nf, halved(nf), "FI_BLOCK_PROLONG"));
		}
	} else if (group == "restrict") {
		for (S nf : {S{17}, S{16}, S{30}}) { small(RESTRICT, nf); }
		small(RESTRICT, S{30, 17});
		for (S nf : {S{64, 30}, S{130, 67}}) {
			v.push_back(make_case(RESTRICT, nf, halved(nf)));
			v.push_back(make_case(RESTRICT, nf, halved(nf), "FI_FLAT_RESTRICT"));
		}
		for (S nf : {S{17, 16, 19}, S{16, 16, 16}}) { small(RESTRICT, nf); }
		for (S nf : {S{30, 17, 19}, S{65, 30, 17}, S{66, 30, 16}, S{64, 16, 17}, S{136, 36, 16}, S{128, 128, 128}, S{128, 128, 127}}) {
			v.push_back(make_case(RESTRICT, nf, halved(nf), nullptr, true));
			v.push_back(make_case(RESTRICT, nf, halved(nf), "FI_ONE_PASS_RESTRICT", true));
			if (nf[0] == 64 || nf[0] == 136) {
				v.push_back(make_case(RESTRICT, nf, halved(nf), "FI_TILED_RESTRICT", true));
				v.push_back(make_case(RESTRICT, nf, halved(nf), "FI_FLAT_RESTRICT", true));
			}
		}
	} else if (group == "slabs") {
		for (S nf : {S{16, 18, 40}, S{17, 16, 41}, S{40, 64}, S{64, 16, 48}}) {
			for (int ranks : {2, 3}) {
				v.push_back(make_case(PROLONG, nf, halved(nf), nullptr, false, ranks));
				if (nf.size() == 3) { v.push_back(make_case(CUBIC, nf, halved(nf), nullptr, false, ranks)); }
				v.push_back(make_case(RESTRICT, nf, halved(nf), nullptr, false, ranks));
				if (nf.size() == 3) { v.push_back(make_case(RESTRICT, nf, halved(nf), nullptr, true, ranks)); }
			}
		}
	} else {
		die("unknown group %s", group.c_str());
	}
	return v;
}

// a rank's slab of the slowest axis: owned planes and local windows (two ghost planes on each side, the storage of
// compute_geom with a halo of 2; level_pair's fields)
struct Slab {
	int f_lo, f_hi, f_base, f_local;
	int c_lo, c_hi, c_base, c_local;
};
Slab slab_of(const Case& c, int r)
{
	const int a = c.ndim - 1, n = c.nf[a], nc = c.nc(a);
	if (c.ranks == 1) { return Slab{0, n, 0, n, 0, nc, 0, nc}; }
	const int H = 2;
	const int lo = static_cast<int>(static_cast<int64_t>(r) * n / c.ranks), hi = static_cast<int>(static_cast<int64_t>(r + 1) * n / c.ranks);
	const int clo = (lo + 1) / 2, chi = (hi + 1) / 2;
	return Slab{lo, hi, lo - H, (hi - lo) + 2 * H, clo, chi, clo - H, (chi - clo) + 2 * H};
}
fi::LevelPair pair_of(const Case& c, const Slab& s)
{
	fi::LevelPair L{};
	L.ndim = c.ndim;
	for (int d = 0; d < 3; ++d) {
		L.nf[d] = c.nf[d];
		L.nc[d] = c.nc(d);
		L.cc[d] = c.cc[d];
	}
	L.f_z0 = s.f_lo;
	L.f_planes = s.f_hi - s.f_lo;
	L.f_base = s.f_base;
	L.c_z0 = s.c_lo;
	L.c_planes = s.c_hi - s.c_lo;
	L.c_base = s.c_base;
	return L;
}

// the kernels the dispatch must pick for a case: the thresholds of launch_prolong / launch_prolong_cubic / launch_restrict
// restated
std::string expected_kernels(const Case& c)
{
	auto sw = [&](const char* name) { return c.sw && std::strcmp(c.sw, name) == 0; };
	const bool whole = c.ranks == 1;
	const int nc0 = c.nc(0), nc1 = c.nc(1), nc2 = c.nc(2);
	if (c.op == PROLONG || c.op == CUBIC) {
		const bool cubic = c.op == CUBIC;
		if (c.ndim == 1) { return "k_prolong"; }
		if (c.ndim == 2) { return "k_prolong2"; }
		const bool rows = c.cc[0] && c.cc[1] && c.cc[2] && nc0 % 2 == 0 && nc0 >= 128 && nc1 >= 64 && nc2 >= 64 && whole && !sw("FI_BLOCK_PROLONG");
		return rows ? (cubic ? "k_prolong3_cubic_rows" : "k_prolong3_rows") : (cubic ? "k_prolong3_cubic" : "k_prolong3");
	}
	if (c.ndim == 1) { return "k_restrict"; }
	if (c.ndim == 2) { return whole && nc0 >= 32 && !sw("FI_FLAT_RESTRICT") ? "k_restrict3_xy_tiled" : "k_restrict2"; }
	if (!c.two_pass || sw("FI_ONE_PASS_RESTRICT")) { return "k_restrict3"; }
	const bool halves = c.cc[0] && c.cc[1] && c.nf[0] % 4 == 0 && nc0 >= 8 && nc1 >= 8;
	std::string k;
	if (halves && nc0 >= 32 && !sw("FI_FLAT_RESTRICT") && !sw("FI_TILED_RESTRICT")) { k = "k_restrict3_xy_rows"; }
	else if (nc0 >= 32 && !sw("FI_FLAT_RESTRICT")) { k = "k_restrict3_xy_tiled"; }
	else { k = "k_restrict3_xy"; }
	// (the z pass sees a rank's owned coarse planes; of the slabs here none reaches 2^18 points)
	const int64_t n_z = static_cast<int64_t>(nc0) * nc1 * (whole ? nc2 : 0);
	return k + (nc0 % 4 == 0 && n_z >= (1 << 18) ? "+k_restrict3_z4" : "+k_restrict3_z");
}

std::string describe(const Case& c)
{
	char buf[256];
	std::string nf = "[", cc = "[";
	for (int d = 0; d < c.ndim; ++d) {
		nf += std::to_string(c.nf[d]) + (d + 1 < c.ndim ? "," : "]");
		cc += std::to_string(c.cc[d]) + (d + 1 < c.ndim ? "," : "]");
	}
	std::snprintf(buf, sizeof buf, "op=%s kernels=%s nf=%s cc=%s ranks=%d switch=%s", c.op == PROLONG ? "prolong" : (c.op == CUBIC ? "cubic" : "restrict"),
	              expected_kernels(c).c_str(), nf.c_str(), cc.c_str(), c.ranks, c.sw ? c.sw : "-");
	return buf;
}

// ---- inputs and reference values of a case ----------------------------------------------------------------------

uint64_t splitmix(uint64_t& s)
{
	uint64_t z = (s += 0x9e3779b97f4a7c15ull);
	z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
	z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
	return z ^ (z >> 31);
}
Vd random_vector(uint64_t seed, size_t n, Kind kind)
{
	Vd v(n);
	uint64_t s = seed;
	for (size_t i = 0; i < n; ++i) {
		if (kind == INT) {
			v[i] = static_cast<double>(static_cast<int>(splitmix(s) % 2001) - 1000);
		} else {
			const double u1 = (static_cast<double>(splitmix(s) >> 11) + 1.0) / 9007199254740993.0, u2 = static_cast<double>(splitmix(s) >> 11) / 9007199254740992.0;
			v[i] = std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
			if (kind == REAL32) { v[i] = static_cast<double>(static_cast<float>(v[i])); }
		}
	}
	return v;
}

struct Ref {
	Vd x;          // the input on the whole lattice (coarse for interpolation, fine for restriction)
	Vd fine0;      // interpolation, mode 1: what the fine vector held
	Vd val, S;     // Op x and sum |w||x|
	Vd val1, S1;   // fine0 + Op x and |fine0| + sum |w||x|
};
std::string ref_key(const Case& c, Kind kind)
{
	char buf[128];
	std::snprintf(buf, sizeof buf, "%d/%d/%d,%d,%d/%d,%d,%d/%d", c.op, c.ndim, c.nf[0], c.nf[1], c.nf[2], c.cc[0], c.cc[1], c.cc[2], kind);
	return buf;
}
std::map<std::string, Ref> g_refs;
std::string g_refs_shape;
const Ref& reference(const Case& c, Kind kind)
{
	char shape[64];
	std::snprintf(shape, sizeof shape, "%d,%d,%d", c.nf[0], c.nf[1], c.nf[2]);
	if (g_refs_shape != shape) {  // (the cases come shape by shape: one shape's references at a time)
		g_refs.clear();
		g_refs_shape = shape;
	}
	const std::string key = ref_key(c, kind);
	auto it = g_refs.find(key);
	if (it != g_refs.end()) { return it->second; }
	Sp  ops[3];
	int din[3] = {1, 1, 1};
	size_t nfine = 1, ncoarse = 1;
	for (int d = 0; d < c.ndim; ++d) {
		const AxisRef A = make_axis(c.nf[d], c.cc[d]);
		ops[d] = sparse(c.op == CUBIC ? A.cub : A.lin, A.nf, A.nc, c.op == RESTRICT);
		din[d] = c.op == RESTRICT ? A.nf : A.nc;
		nfine *= A.nf;
		ncoarse *= A.nc;
	}
	uint64_t seed = 0x5eed;
	for (char ch : key) { seed = seed * 1099511628211ull + static_cast<unsigned char>(ch); }
	Ref R;
	R.x = random_vector(seed, c.op == RESTRICT ? nfine : ncoarse, kind);
	Vd ax(R.x.size());
	for (size_t i = 0; i < ax.size(); ++i) { ax[i] = std::fabs(R.x[i]); }
	R.val = apply3(ops, din, R.x, false);
	R.S   = apply3(ops, din, ax, true);
	if (c.op == PROLONG) {
		R.fine0 = random_vector(seed ^ 0xf17eull, nfine, kind);
		R.val1.resize(nfine);
		R.S1.resize(nfine);
		for (size_t i = 0; i < nfine; ++i) {
			R.val1[i] = R.fine0[i] + R.val[i];
			R.S1[i]   = std::fabs(R.fine0[i]) + R.S[i];
		}
	}
	return g_refs.emplace(key, std::move(R)).first->second;
}

// ---- the device side ---------------------------------------------------------------------------------------------

template <typename T> T sentinel();
template <> float sentinel<float>() { const uint32_t b = 0x7fc5a5a5u; float v; std::memcpy(&v, &b, 4); return v; }
template <> double sentinel<double>() { const uint64_t b = 0x7ff85a5a5a5a5a5aull; double v; std::memcpy(&v, &b, 8); return v; }
template <typename T> bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// a device array between two guard zones of 64 elements, with its host image
template <typename T>
struct Buf {
	static constexpr size_t G = 64;
	std::vector<T> h;
	T* d = nullptr;
	size_t n;
	Buf(size_t n_, T fill) : h(n_ + 2 * G, fill), n(n_) { HIP_OK(hipMalloc(reinterpret_cast<void**>(&d), h.size() * sizeof(T))); }
	Buf(const Buf&) = delete;
	~Buf() { HIP_OK(hipFree(d)); }
	T* host() { return h.data() + G; }
	T* dev() { return d + G; }
	void up() { HIP_OK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)); }
	void down() { HIP_OK(hipMemcpy(h.data(), d, h.size() * sizeof(T), hipMemcpyDeviceToHost)); }
	bool guards_hold(T fill) const
	{
		for (size_t i = 0; i < G; ++i) {
			if (!same_bits(h[i], fill) || !same_bits(h[G + n + i], fill)) { return false; }
		}
		return true;
	}
};

constexpr double kGarbage = 4242.0;  // ghost planes beyond the lattice and the guards of inputs: finite, never to be drawn on

// the local window of planes base .. base + local of a lattice vector (planes outside the lattice: kGarbage)
template <typename T>
void fill_window(Buf<T>& b, const Vd& global, size_t pe, int base, int local, int n)
{
	for (int p = 0; p < local; ++p) {
		const int g = base + p;
		for (size_t e = 0; e < pe; ++e) { b.host()[p * pe + e] = (g >= 0 && g < n) ? static_cast<T>(global[g * pe + e]) : static_cast<T>(kGarbage); }
	}
}

struct Tally {
	double max_ratio = 0;
};
std::map<std::string, double> g_ratios;  // "<kernels> <arithmetic>" -> the largest |got - ref| / (u sum |w||x|)

// the owned planes of a local output array against the reference on the whole lattice; everything else keeps the sentinel
template <typename TO>
void check_output(const std::string& what, Buf<TO>& out, size_t pe, int local, int own0, int owned, int g0, const Vd& ref, const Vd& S, bool exact,
                  double k, double u, Tally& tally)
{
	const TO sen = sentinel<TO>();
	REQUIRE(out.guards_hold(sen), "%s: a write outside the output array", what.c_str());
	long bad = 0;
	for (int p = 0; p < local; ++p) {
		const bool mine = p >= own0 && p < own0 + owned;
		for (size_t e = 0; e < pe; ++e) {
			const TO got = out.host()[p * pe + e];
			if (!mine) {
				if (!same_bits(got, sen) && bad++ == 0) { std::printf("%s: local plane %d element %zu is not owned and was written (%g)\n", what.c_str(), p, e, static_cast<double>(got)); }
				continue;
			}
			const size_t gi = static_cast<size_t>(g0 + p - own0) * pe + e;
			const double g = static_cast<double>(got), r = ref[gi], s = S[gi];
			bool ok;
			if (exact) {
				ok = same_bits(got, static_cast<TO>(r));  // (the reference's numbers are multiples of 2^-6 / 2^-24: TO holds them)
			} else {
				const double err = std::fabs(g - r);
				ok = err <= k * u * s;  // (false for a NaN)
				if (ok && s > 0 && err / (u * s) > tally.max_ratio) { tally.max_ratio = err / (u * s); }
			}
			if (!ok && bad++ == 0) {
				std::printf("%s: global plane %d element %zu: got %.17g, reference %.17g, sum|w||x| %.17g (%s)\n", what.c_str(), g0 + p - own0, e, g, r, s,
				            exact ? "equal bits required" : "outside k u sum|w||x|");
			}
		}
	}
	REQUIRE(bad == 0, "%s: %ld wrong elements", what.c_str(), bad);
}

hipStream_t g_stream = nullptr;

void set_switch(const char* name)
{
	for (const char* s : kSwitches) { unsetenv(s); }
	if (name) { setenv(name, "1", 1); }
}

template <typename T> const char* type_name();
template <> const char* type_name<float>() { return "f32"; }
template <> const char* type_name<double>() { return "f64"; }

// one case in one precision, on one kind of input (and one mode): every rank's launch, checked
template <typename T, typename TO>
void run(const std::string& group, const Case& c, Kind kind, int mode)
{
	const Ref& R = reference(c, kind);
	const int a = c.ndim - 1;
	size_t pe_f = 1, pe_c = 1;
	for (int d = 0; d < a; ++d) { pe_f *= c.nf[d]; pe_c *= c.nc(d); }
	const double u = std::is_same<T, float>::value ? std::ldexp(1.0, -24) : std::ldexp(1.0, -53);  // the ARITHMETIC's unit (TO only widens the store)
	const double k = c.op == PROLONG ? 8 + 3 : (c.op == CUBIC ? 64 + 4 : 125 + 3);
	const bool exact = kind == INT && (c.op != CUBIC || std::is_same<T, double>::value);
	char what[384];
	std::snprintf(what, sizeof what, "%s type=%s%s%s input=%s mode=%d", describe(c).c_str(), type_name<T>(), c.op == CUBIC ? "->" : "",
	              c.op == CUBIC ? type_name<TO>() : "", kind == INT ? "int" : "real", mode);
	Tally tally;
	for (int r = 0; r < c.ranks; ++r) {
		const Slab s = slab_of(c, r);
		const fi::LevelPair L = pair_of(c, s);
		const std::string w = std::string(what) + " rank=" + std::to_string(r);
		if (c.op == RESTRICT) {
			Buf<T> fine(pe_f * s.f_local, static_cast<T>(kGarbage)), coarse(pe_c * s.c_local, sentinel<T>());
			fill_window(fine, R.x, pe_f, s.f_base, s.f_local, c.nf[a]);
			fine.up();
			coarse.up();
			const bool tp = c.two_pass;
			Buf<T> tmp(tp ? pe_c * s.f_local : 1, sentinel<T>());  // (scratch: its contents are not checked, its guards are)
			tmp.up();
			set_switch(c.sw);
			fi::launch_restrict<T>(L, fine.dev(), coarse.dev(), g_stream, tp ? tmp.dev() : nullptr, tp ? s.f_local : 0);
			set_switch(nullptr);
			HIP_OK(hipGetLastError());
			HIP_OK(hipStreamSynchronize(g_stream));
			coarse.down();
			tmp.down();
			REQUIRE(tmp.guards_hold(sentinel<T>()), "%s: a write outside the work array", w.c_str());
			check_output<T>(w, coarse, pe_c, s.c_local, s.c_lo - s.c_base, s.c_hi - s.c_lo, s.c_lo, R.val, R.S, exact, k, u, tally);
		} else {
			Buf<T>  coarse(pe_c * s.c_local, static_cast<T>(kGarbage));
			Buf<TO> fine(pe_f * s.f_local, sentinel<TO>());
			fill_window(coarse, R.x, pe_c, s.c_base, s.c_local, c.nc(a));
			if (mode) {  // the owned points hold the vector that is added onto
				for (int p = s.f_lo; p < s.f_hi; ++p) {
					for (size_t e = 0; e < pe_f; ++e) { fine.host()[(p - s.f_base) * pe_f + e] = static_cast<TO>(R.fine0[p * pe_f + e]); }
				}
			}
			coarse.up();
			fine.up();
			set_switch(c.sw);
			if (c.op == CUBIC) { fi::launch_prolong_cubic<T, TO>(L, coarse.dev(), fine.dev(), g_stream); }
			else { fi::launch_prolong<T>(L, coarse.dev(), reinterpret_cast<T*>(fine.dev()), mode, g_stream); }
			set_switch(nullptr);
			HIP_OK(hipGetLastError());
			HIP_OK(hipStreamSynchronize(g_stream));
			fine.down();
			check_output<TO>(w, fine, pe_f, s.f_local, s.f_lo - s.f_base, s.f_hi - s.f_lo, s.f_lo, mode ? R.val1 : R.val, mode ? R.S1 : R.S, exact, k, u, tally);
		}
	}
	if (exact) {
		std::printf("case %s %s: equal bits\n", group.c_str(), what);
	} else {
		std::printf("case %s %s: within %g u sum|w||x|, largest ratio %.3f\n", group.c_str(), what, k, tally.max_ratio);
		double& m = g_ratios[expected_kernels(c) + " " + type_name<T>()];
		m = tally.max_ratio > m ? tally.max_ratio : m;
	}
	std::fflush(stdout);
}

void run_group(const std::string& group)
{
	HIP_OK(hipSetDevice(0));
	HIP_OK(hipStreamCreate(&g_stream));
	for (const Case& c : cases_of(group)) {
		for (int real = 0; real < 2; ++real) {
			const Kind k32 = real ? REAL32 : INT, k64 = real ? REAL64 : INT;
			if (c.op == CUBIC) {
				run<float, float>(group, c, k32, 0);
				run<double, double>(group, c, k64, 0);
				run<float, double>(group, c, k32, 0);
			} else {
				for (int mode = 0; mode < (c.op == PROLONG ? 2 : 1); ++mode) {
					run<float, float>(group, c, k32, mode);
					run<double, double>(group, c, k64, mode);
				}
			}
		}
	}
	HIP_OK(hipStreamSynchronize(g_stream));
	HIP_OK(hipStreamDestroy(g_stream));
	for (const auto& kv : g_ratios) { std::printf("ratio %s %s %.3f\n", group.c_str(), kv.first.c_str(), kv.second); }
}

// the reference on its own, and the premise of the equal-bits comparisons (no HIP call)
void run_host()
{
	for (int nf = 15; nf <= 70; ++nf) {
		check_axis(make_axis(nf, 0));
		if (nf % 2 == 0) { check_axis(make_axis(nf, 1)); }
	}
	std::printf("host: rows, linear and cubic exactness hold for the extents 15 .. 70, both halvings\n");
	double worst_lin = 0, worst_cub = 0;
	for (const char* group : {"prolong", "cubic", "restrict", "slabs"}) {
		for (const Case& c : cases_of(group)) {
			std::printf("plan %s %s\n", group, describe(c).c_str());
			const Ref& R = reference(c, INT);
			const Vd&  S = c.op == PROLONG ? R.S1 : R.S;  // (mode 1 has the larger sums)
			double m = 0;
			for (double s : S) { m = s > m ? s : m; }
			for (double v : (c.op == PROLONG ? R.val1 : R.val)) {
				REQUIRE(std::ldexp(v, c.op == CUBIC ? 24 : 6) == std::nearbyint(std::ldexp(v, c.op == CUBIC ? 24 : 6)), "%s: a result off the lattice of exact sums", describe(c).c_str());
			}
			if (c.op == CUBIC) {
				REQUIRE(std::ldexp(m, 24) < std::ldexp(1.0, 53), "%s: 2^24 max sum|w x| = %g is not below 2^53", describe(c).c_str(), std::ldexp(m, 24));
				worst_cub = m > worst_cub ? m : worst_cub;
			} else {
				REQUIRE(64.0 * m < std::ldexp(1.0, 24), "%s: 64 max sum|w x| = %g is not below 2^24", describe(c).c_str(), 64.0 * m);
				worst_lin = m > worst_lin ? m : worst_lin;
			}
		}
	}
	std::printf("host: 64 max sum|w x| = %.0f < 2^24 (linear interpolation, restriction); 2^24 max sum|w x| = %.6g < 2^53 (cubic)\n", 64.0 * worst_lin,
	            std::ldexp(worst_cub, 24));
}

}  // namespace

int main(int argc, char** argv)
{
	if (argc != 2) { die("usage: %s host|prolong|cubic|restrict|slabs", argv[0]); }
	const std::string group = argv[1];
	set_switch(nullptr);
	if (group == "host") { run_host(); }
	else { run_group(group); }
	std::printf("all %s checks passed\n", group.c_str());
	return 0;
}
