// fi_sample.hip -- values and gradients of a lattice field at arbitrary points, on the device.
//
// The contract (include/fi_hip.h fi_sample): positions in global lattice coordinates; a point inside the
// lattice takes the cell c_d = min(floor(p_d), n_d - 2) and the offset t_d = p_d - c_d in [0, 1].  FI_SAMPLE_LINEAR is the
// multilinear kernel of the reference's value rows (multilerp, field_interpolation.cpp:15-55), FI_SAMPLE_CUBIC is Catmull-Rom
// over the samples c - 1 .. c + 2 with clamped indices (the SDF app's bicubic_upsample), both in a fixed order of operations
// so that the numpy oracle (tests/sample_reference.py) matches them bit for bit; -ffp-contract=off keeps every product and
// sum rounded on its own.  One thread per point: the gather is latency-bound, so all of a point's loads are issued before
// the first use (cubic 3-D: one z-plane of 16 at a time, which keeps the fp64 kernel out of scratch).
//
// Slabs (one per process, or the members of a loop-back group): every slab exchanges the ghost planes the mode reads (1 for
// linear, 2 for cubic), samples the points whose slowest cell index lies in its slab and writes -0.0 for every other point;
// the sum over the slabs is then exact, sign of zero included, and points outside the lattice get `fill` after it.
#include "fi_solver_internal.h"
#include "fi_stage.h"
#include "fi_sample.h"

namespace fi {

namespace {

constexpr int kSampleThreads = 256;

// one launch: the field as seen from global plane `first` of the slowest axis, and the cells along that axis it owns
template <typename T>
struct SampleArgs {
	const T*     f;
	int          n[3];      // global extents (1 beyond ndim)
	int          first;     // global slowest-axis plane of f[0]
	int          clo, chi;  // this launch's points: slowest cell index in [clo, chi)
	int          slab;      // 1: points outside the lattice write -0.0 as well (fill follows the sum over the slabs)
	float        fill;
	int64_t      npts;
	const float* pos;       // float[npts][D]
	float*       val;       // float[npts]
	float*       grad;      // float[npts][D], or nullptr
};

// Catmull-Rom through p0 .. p3, in the contract's order of operations
template <typename T>
struct CatmullRom {
	T p1, a, b, e;
	__device__ CatmullRom(T p0, T q1, T p2, T p3)
	    : p1(q1), a(p2 - p0), b(((T(2) * p0 - T(5) * q1) + T(4) * p2) - p3), e((T(3) * (q1 - p2) + p3) - p0)
	{
	}
	// ht = 0.5 * t, t3 = 3 * t
	__device__ T val(T t, T ht) const { return p1 + ht * (a + t * (b + t * e)); }
	__device__ T der(T t, T t3) const { return T(0.5) * (a + t * (T(2) * b + t3 * e)); }
};

template <int D, bool GRAD, typename T>
__device__ inline void store(const SampleArgs<T>& a, int64_t i, float v, const float* g)
{
	a.val[i] = v;
	if (GRAD) {
#pragma unroll
		for (int d = 0; d < D; ++d) { a.grad[i * D + d] = g[d]; }
	}
}

template <int D, int MODE, typename T, bool GRAD>
__global__ __launch_bounds__(kSampleThreads) void k_sample(SampleArgs<T> a)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kSampleThreads + threadIdx.x;
	if (i >= a.npts) { return; }
	float p[D];
#pragma unroll
	for (int d = 0; d < D; ++d) { p[d] = a.pos[i * D + d]; }
	bool in = true;
#pragma unroll
	for (int d = 0; d < D; ++d) { in = in && p[d] >= 0.0f && p[d] <= static_cast<float>(a.n[d] - 1); }  // (NaN fails both)
	int c[D];
#pragma unroll
	for (int d = 0; d < D; ++d) { c[d] = in ? min(static_cast<int>(floorf(p[d])), a.n[d] - 2) : 0; }
	float out[1 + D];
	if (!in || c[D - 1] < a.clo || c[D - 1] >= a.chi) {
		const float other = in || a.slab ? -0.0f : a.fill;
#pragma unroll
		for (int k = 0; k <= D; ++k) { out[k] = other; }
		store<D, GRAD>(a, i, out[0], out + 1);
		return;
	}
	T t[D];
#pragma unroll
	for (int d = 0; d < D; ++d) { t[d] = static_cast<T>(p[d]) - static_cast<T>(c[d]); }
	// strides of the global lattice; the slowest axis counts from plane `first`
	int64_t s[D];
	s[0] = 1;
#pragma unroll
	for (int d = 1; d < D; ++d) { s[d] = s[d - 1] * a.n[d - 1]; }
	const T* f = a.f;

	if constexpr (MODE == FI_SAMPLE_LINEAR) {
		int64_t o = 0;
#pragma unroll
		for (int d = 0; d < D; ++d) { o += s[d] * (d == D - 1 ? c[d] - a.first : c[d]); }
		T fv[1 << D];
#pragma unroll
		for (int k = 0; k < (1 << D); ++k) {
			int64_t q = o;
#pragma unroll
			for (int d = 0; d < D; ++d) {
				if ((k >> d) & 1) { q += s[d]; }
			}
			fv[k] = f[q];
		}
		T u[D][2];
#pragma unroll
		for (int d = 0; d < D; ++d) {
			u[d][0] = T(1) - t[d];
			u[d][1] = t[d];
		}
		T v = T(0);
#pragma unroll
		for (int k = 0; k < (1 << D); ++k) {
			T w = u[0][k & 1];
#pragma unroll
			for (int d = 1; d < D; ++d) { w = w * u[d][(k >> d) & 1]; }
			const T term = w * fv[k];
			v = k == 0 ? term : v + term;
		}
		out[0] = static_cast<float>(v);
		if constexpr (GRAD) {
#pragma unroll
			for (int d = 0; d < D; ++d) {
				T    g = T(0);
				bool first = true;
#pragma unroll
				for (int k = 0; k < (1 << D); ++k) {
					if ((k >> d) & 1) { continue; }
					T term = fv[k | (1 << d)] - fv[k];
					if (D > 1) {
						T    W = T(1);
						bool have = false;
#pragma unroll
						for (int e = 0; e < D; ++e) {
							if (e == d) { continue; }
							W    = have ? W * u[e][(k >> e) & 1] : u[e][(k >> e) & 1];
							have = true;
						}
						term = W * term;
					}
					g     = first ? term : g + term;
					first = false;
				}
				out[1 + d] = static_cast<float>(g);
			}
		}
	} else {
		// clamped sample offsets c - 1 .. c + 2 per axis
		int64_t o[D][4];
		T       ht[D], t3[D];
#pragma unroll
		for (int d = 0; d < D; ++d) {
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				const int x = min(max(c[d] - 1 + k, 0), a.n[d] - 1);
				o[d][k]     = s[d] * (d == D - 1 ? x - a.first : x);
			}
			ht[d] = T(0.5) * t[d];
			t3[d] = T(3) * t[d];
		}
		if constexpr (D == 1) {
			const CatmullRom<T> cx(f[o[0][0]], f[o[0][1]], f[o[0][2]], f[o[0][3]]);
			out[0] = static_cast<float>(cx.val(t[0], ht[0]));
			if constexpr (GRAD) { out[1] = static_cast<float>(cx.der(t[0], t3[0])); }
		} else {
			// one plane of 4 x 4 samples (rows along x at the 4 y offsets), reduced along x then y: P (value), GX (CR' along
			// x), GY (CR' along y)
			auto plane = [&](int64_t oz, T* P, T* GX, T* GY) {
				T fv[4][4];
#pragma unroll
				for (int j = 0; j < 4; ++j) {
#pragma unroll
					for (int k = 0; k < 4; ++k) { fv[j][k] = f[oz + o[1][j] + o[0][k]]; }
				}
				T r[4], dr[4];
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const CatmullRom<T> cx(fv[j][0], fv[j][1], fv[j][2], fv[j][3]);
					r[j] = cx.val(t[0], ht[0]);
					if (GRAD) { dr[j] = cx.der(t[0], t3[0]); }
				}
				const CatmullRom<T> cy(r[0], r[1], r[2], r[3]);
				*P = cy.val(t[1], ht[1]);
				if (GRAD) {
					*GX = CatmullRom<T>(dr[0], dr[1], dr[2], dr[3]).val(t[1], ht[1]);
					*GY = cy.der(t[1], t3[1]);
				}
			};
			if constexpr (D == 2) {
				T P, GX = T(0), GY = T(0);
				plane(0, &P, &GX, &GY);
				out[0] = static_cast<float>(P);
				if constexpr (GRAD) {
					out[1] = static_cast<float>(GX);
					out[2] = static_cast<float>(GY);
				}
			} else {
				T P[4], GX[4] = {}, GY[4] = {};
#pragma unroll
				for (int m = 0; m < 4; ++m) { plane(o[2][m], &P[m], &GX[m], &GY[m]); }
				const CatmullRom<T> cz(P[0], P[1], P[2], P[3]);
				out[0] = static_cast<float>(cz.val(t[2], ht[2]));
				if constexpr (GRAD) {
					out[1] = static_cast<float>(CatmullRom<T>(GX[0], GX[1], GX[2], GX[3]).val(t[2], ht[2]));
					out[2] = static_cast<float>(CatmullRom<T>(GY[0], GY[1], GY[2], GY[3]).val(t[2], ht[2]));
					out[3] = static_cast<float>(cz.der(t[2], t3[2]));
				}
			}
		}
	}
	store<D, GRAD>(a, i, out[0], out + 1);
}

// after the sum over the slabs: `fill` at the points outside the lattice
template <int D>
__global__ __launch_bounds__(kSampleThreads) void k_sample_fill(int64_t npts, const float* __restrict__ pos, int n0, int n1, int n2,
                                                                 float fill, float* __restrict__ val, float* __restrict__ grad)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kSampleThreads + threadIdx.x;
	if (i >= npts) { return; }
	const int n[3] = {n0, n1, n2};
	bool in = true;
#pragma unroll
	for (int d = 0; d < D; ++d) {
		const float p = pos[i * D + d];
		in = in && p >= 0.0f && p <= static_cast<float>(n[d] - 1);
	}
	if (in) { return; }
	val[i] = fill;
	if (grad) {
#pragma unroll
		for (int d = 0; d < D; ++d) { grad[i * D + d] = fill; }
	}
}

// a loop-back group member's results into member 0's: one of the two is -0.0, so the sum is exact
__global__ __launch_bounds__(kSampleThreads) void k_sample_add(int64_t n, const float* __restrict__ src, float* __restrict__ dst)
{
	const int64_t i = static_cast<int64_t>(blockIdx.x) * kSampleThreads + threadIdx.x;
	if (i < n) { dst[i] += src[i]; }
}

inline dim3 sample_blocks(int64_t n) { return dim3(static_cast<unsigned>((n + kSampleThreads - 1) / kSampleThreads)); }

template <int D, int MODE, typename T>
void launch_dm(const SampleArgs<T>& a, hipStream_t st)
{
	if (a.grad) {
		hipLaunchKernelGGL((k_sample<D, MODE, T, true>), sample_blocks(a.npts), dim3(kSampleThreads), 0, st, a);
	} else {
		hipLaunchKernelGGL((k_sample<D, MODE, T, false>), sample_blocks(a.npts), dim3(kSampleThreads), 0, st, a);
	}
	FI_HIP_TRY(hipGetLastError());
}

template <int D, typename T>
void launch_d(int mode, const SampleArgs<T>& a, hipStream_t st)
{
	if (mode == FI_SAMPLE_LINEAR) {
		launch_dm<D, FI_SAMPLE_LINEAR>(a, st);
	} else {
		launch_dm<D, FI_SAMPLE_CUBIC>(a, st);
	}
}

template <typename T>
void launch(int ndim, int mode, const SampleArgs<T>& a, hipStream_t st)
{
	if (a.npts == 0) { return; }
	if (ndim == 1) {
		launch_d<1>(mode, a, st);
	} else if (ndim == 2) {
		launch_d<2>(mode, a, st);
	} else {
		launch_d<3>(mode, a, st);
	}
}

void check_query(int ndim, const int* sizes, int64_t n, const float* positions, int mode, const float* values, int memory)
{
	FI_REQUIRE(n >= 0, FI_ERR_INVALID, "n = %lld", static_cast<long long>(n));
	FI_REQUIRE(positions != nullptr && values != nullptr, FI_ERR_INVALID, "null positions or values");
	FI_REQUIRE(mode == FI_SAMPLE_LINEAR || mode == FI_SAMPLE_CUBIC, FI_ERR_INVALID, "bad sampling mode %d", mode);
	check_memory(memory);
	FI_REQUIRE(sizes != nullptr, FI_ERR_INVALID, "sizes is null");
	FI_REQUIRE(ndim >= 1 && ndim <= 3, FI_ERR_INVALID, "ndim must be 1, 2 or 3 (got %d)", ndim);
	for (int d = 0; d < ndim; ++d) { FI_REQUIRE(sizes[d] >= 2, FI_ERR_INVALID, "sampling needs sizes >= 2 (sizes[%d] = %d)", d, sizes[d]); }
	// (one thread per point: the grid stays below 2^32 threads)
	FI_REQUIRE(n < (int64_t(1) << 31), FI_ERR_UNSUPPORTED, "%lld points in one call", static_cast<long long>(n));
}

// the call's buffers on the device (fi_stage.h), its kernel arguments, and finish(), which copies back and ends the call
struct Query {
	int64_t           n;
	int               D;
	stage::In<float>  pos;
	stage::Out<float> val, grad;
	Query(int ndim, int64_t npts, const float* positions, float* values, float* gradients, int memory, hipStream_t st)
	    : n(npts), D(ndim), pos(positions, D * n, memory, st), val(values, n, memory), grad(gradients, D * n, memory)
	{
	}
	template <typename T>
	SampleArgs<T> args(const T* f, const int* sizes, float fill) const
	{
		SampleArgs<T> a{};
		a.f = f;
		for (int d = 0; d < 3; ++d) { a.n[d] = d < D ? sizes[d] : 1; }
		a.first = 0;
		a.clo   = 0;
		a.chi   = sizes[D - 1];
		a.slab  = 0;
		a.fill  = fill;
		a.npts  = n;
		a.pos   = pos;
		a.val   = val;
		a.grad  = grad;
		return a;
	}
	void finish(hipStream_t st)
	{
		val.back(st);
		grad.back(st);
		FI_HIP_TRY(hipStreamSynchronize(st));
	}
};

// Slab contexts: one per process (RankSet of one, ghost planes over RCCL or the host test transport, results summed by
// allreduce_sum_vec) or all members of a loop-back group (device copies, results summed into member 0's).  fields[r]:
// member r's owned values (fp32, `memory`), or nullptr for its last solution.  As fi_iso.hip's slab_pieces: the values go
// into the work vector q in the member's local layout and the ghost planes the mode reads are exchanged; every rank
// exchanges the same width and applies the same rule, decided from facts all ranks share.  whole (a loop-back group whose
// caller holds the whole lattice, on the device): every member samples its points from it, nothing to exchange.
void slab_sample(RankSet& R, const float* const* fields, const float* whole, int memory, int64_t n, const float* positions,
                 int mode, float fill, float* values, float* gradients)
{
	fi_ctx*     c0 = R[0];
	const Geom& g0 = c0->g;
	const int   D  = g0.ndim;
	const int   L  = D - 1;
	const int   want = mode == FI_SAMPLE_CUBIC ? 2 : 1;
	FI_REQUIRE(whole || (c0->halo >= want && g0.gn[L] / c0->nranks >= want), FI_ERR_UNSUPPORTED,
	           "%s sampling over slabs needs %d ghost planes and slabs of at least %d planes (the context stores %d ghost "
	           "planes, the thinnest slab has %d planes)", mode == FI_SAMPLE_CUBIC ? "cubic" : "linear", want, want, c0->halo,
	           g0.gn[L] / c0->nranks);
	for (size_t r = 0; r < R.size(); ++r) { FI_REQUIRE(whole || fields[r] || R[r]->vectors_ready, FI_ERR_STATE, "no solution yet"); }
	if (n == 0) { return; }
	AllocStream alloc_on(c0->stream);
	Query q(D, n, positions, values, gradients, memory, c0->stream);
	if (!whole) { slab_fields(R, fields, memory, want); }  // (no member is without a field: checked above, before n == 0 returns)
	DevBuf buf, sval, sgrad;  // an fp64 member's values rounded to fp32; members 1.. before they are added to member 0's
	if (R.size() > 1) {
		sval.alloc(sizeof(float) * n);
		if (q.grad) { sgrad.alloc(sizeof(float) * D * n); }
	}
	for (size_t r = 0; r < R.size(); ++r) {
		fi_ctx*     c = R[r];
		const Geom& g = c->g;
		float*      v  = r == 0 ? q.val : sval.as<float>();
		float*      gr = q.grad == nullptr ? nullptr : (r == 0 ? q.grad : sgrad.as<float>());
		auto finish_args = [&](auto a) {
			a.first = g.off[L];
			a.clo   = c->slab_lo;
			a.chi   = c->slab_hi;
			a.slab  = 1;
			a.val   = v;
			a.grad  = gr;
			launch(D, mode, a, c->stream);
		};
		if (whole) {
			auto a  = q.args<float>(whole, g.gn, fill);
			a.clo   = c->slab_lo;
			a.chi   = c->slab_hi;
			a.slab  = 1;
			a.val   = v;
			a.grad  = gr;
			launch(D, mode, a, c->stream);
		} else if (!fields[r] && c->dtype == FI_F64) {  // the fp64 solution, sampled in fp64
			finish_args(q.args<double>(c->q.as<double>(), g.gn, fill));
		} else if (c->dtype == FI_F64) {  // fp32 values passed in: widened exactly by load_owned, narrowed back exactly here
			buf.alloc(sizeof(float) * g.nloc);
			hipLaunchKernelGGL((k_to_float<double>), dim3(blocks_for(g.nloc)), dim3(kThreads), 0, c->stream, g.nloc, c->q.as<double>(),
			                   buf.as<float>());
			FI_HIP_TRY(hipGetLastError());
			finish_args(q.args<float>(buf.as<float>(), g.gn, fill));
		} else {
			finish_args(q.args<float>(c->q.as<float>(), g.gn, fill));
		}
		if (r > 0) {
			hipLaunchKernelGGL(k_sample_add, sample_blocks(n), dim3(kSampleThreads), 0, c->stream, n, sval.as<float>(), q.val);
			if (q.grad) {
				hipLaunchKernelGGL(k_sample_add, sample_blocks(D * n), dim3(kSampleThreads), 0, c->stream, D * n, sgrad.as<float>(),
				                   q.grad);
			}
			FI_HIP_TRY(hipGetLastError());
		}
	}
	if (R.size() == 1) {
		allreduce_sum_vec(c0, q.val, n, false);
		if (q.grad) { allreduce_sum_vec(c0, q.grad, D * n, false); }
	}
	const int* gn = g0.gn;
	const int  n1 = D > 1 ? gn[1] : 1, n2 = D > 2 ? gn[2] : 1;
	if (D == 1) {
		hipLaunchKernelGGL((k_sample_fill<1>), sample_blocks(n), dim3(kSampleThreads), 0, c0->stream, n, q.pos, gn[0], n1, n2, fill, q.val, q.grad);
	} else if (D == 2) {
		hipLaunchKernelGGL((k_sample_fill<2>), sample_blocks(n), dim3(kSampleThreads), 0, c0->stream, n, q.pos, gn[0], n1, n2, fill, q.val, q.grad);
	} else {
		hipLaunchKernelGGL((k_sample_fill<3>), sample_blocks(n), dim3(kSampleThreads), 0, c0->stream, n, q.pos, gn[0], n1, n2, fill, q.val, q.grad);
	}
	FI_HIP_TRY(hipGetLastError());
	q.finish(c0->stream);
}

}  // namespace

void sample_field(const float* field, int ndim, const int* sizes, int64_t n, const float* positions, int mode, float fill,
                  float* values, float* gradients, int memory)
{
	FI_REQUIRE(field != nullptr, FI_ERR_INVALID, "field is null");
	check_query(ndim, sizes, n, positions, mode, values, memory);
	if (n == 0) { return; }
	hipStream_t st = nullptr;
	Query q(ndim, n, positions, values, gradients, memory, st);
	int64_t total = 1;
	for (int d = 0; d < ndim; ++d) { total *= sizes[d]; }
	stage::In<float> f(field, total, memory, st);
	launch(ndim, mode, q.args<float>(f, sizes, fill), st);
	q.finish(st);
}

void sample_ctx(fi_ctx* c, const float* field, int64_t n, const float* positions, int mode, float fill, float* values,
                float* gradients, int memory)
{
	const Geom& g = c->g;
	check_query(g.ndim, g.gn, n, positions, mode, values, memory);
	if (c->nranks > 1) {
		RankSet R{c};
		slab_sample(R, &field, nullptr, memory, n, positions, mode, fill, values, gradients);
		return;
	}
	FI_REQUIRE(field || c->vectors_ready, FI_ERR_STATE, "no solution yet");
	if (n == 0) { return; }
	AllocStream alloc_on(c->stream);
	Query q(g.ndim, n, positions, values, gradients, memory, c->stream);
	if (!field && c->dtype == FI_F64) {  // the fp64 solution, sampled in fp64
		launch(g.ndim, mode, q.args<double>(owned<double>(c, c->x), g.gn, fill), c->stream);
	} else {
		DevBuf       buf;
		const float* f = field_f32(c, field, memory, buf);
		launch(g.ndim, mode, q.args<float>(f, g.gn, fill), c->stream);
		q.finish(c->stream);  // (before buf goes)
		return;
	}
	q.finish(c->stream);
}

void sample_group(std::vector<fi_ctx*>& members, const float* whole, int64_t n, const float* positions, int mode, float fill,
                  float* values, float* gradients)
{
	fi_ctx* c0 = members[0];
	if (c0->nranks == 1) {  // a group of one: the undivided context
		sample_ctx(c0, whole, n, positions, mode, fill, values, gradients, FI_HOST);
		return;
	}
	const Geom& g = c0->g;
	check_query(g.ndim, g.gn, n, positions, mode, values, FI_HOST);
	if (whole && n == 0) { return; }
	std::vector<const float*> none(members.size(), nullptr);
	DevBuf buf;
	if (whole) {  // the caller holds the whole lattice: every member reads its points' samples from it
		int64_t total = 1;
		for (int d = 0; d < g.ndim; ++d) { total *= g.gn[d]; }
		AllocStream alloc_on(c0->stream);
		buf.alloc(sizeof(float) * total);
		FI_HIP_TRY(hipMemcpyAsync(buf.p, whole, sizeof(float) * total, hipMemcpyHostToDevice, c0->stream));
	}
	slab_sample(members, none.data(), whole ? buf.as<float>() : nullptr, FI_HOST, n, positions, mode, fill, values, gradients);
}

}  // namespace fi
