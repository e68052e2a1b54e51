// fi_robust.hip -- robust fits: iteratively reweighted least squares on the device (include/fi_hip.h, "robust fits";
// DESIGN.md 4.10).  One reweighting step:
//
//   1. k_point_residual   one thread per data point: the point's rows at unit point weight (fi_rows.h, the very function
//                         k_emit_rows writes the row tables with) applied to the field; r = the root of the sum of their
//                         squared residuals, -1 for a point without rows.  A latency-bound gather of 2^D corners per row.
//   2. the median         r >= 0 as a float has an order-preserving bit pattern: the keys (points without rows: all ones, behind
//                         every residual) are sorted by fi_sort.h's Onesweep and the element of rank (M - 1) / 2 is picked on
//                         the device (k_pick_scale); M was counted by the residual pass.
//   3. k_robust_weights   omega and the new point weight base * sqrt(omega) in one pass; max |omega - omega_old| and the
//                         count of omega = 0 by wave reductions into the step's record (integer atomics: the results do
//                         not depend on the order of arrival).
//   4. re-emission        the context's row tables go back to their pool and every batch is emitted again from its
//                         PointBatch: the path and the order of the first emission.
//
// The host reads the record once per step.  Nothing else travels.

#include "fi_sort.h"

#include "fi_internal.h"
#include "fi_robust.h"
#include "fi_rows.h"
#include "fi_solver_internal.h"

namespace fi {

namespace {

struct RobustRecord {
	unsigned int m;          // points with r >= 0
	unsigned int zeroed;     // ... whose omega is 0
	unsigned int dmax_bits;  // max |omega - omega_old| (the bits of a non-negative float order as the float does)
	float        scale;      // s
};

__device__ inline float  root(float v) { return sqrtf(v); }
__device__ inline double root(double v) { return sqrt(v); }

// a point's rows applied to the field: e = sum_q c[q] x[corner q] - b in T, left to right over the corners inside the lattice
template <int D, typename T>
struct RowResidual {
	const T* __restrict__ x;  // the owned values of an undivided lattice, x fastest
	const Geom* g;
	uint32_t    invalid;
	T           ss;
	bool        any;
	__device__ void row(int, uint32_t k, const int* origin, const float* c, float b)
	{
		constexpr int NC = 1 << D;
		if (k == invalid) { return; }
		T e = T(0);
		for (int q = 0; q < NC; ++q) {
			bool    in  = true;
			int64_t idx = 0, mul = 1;
			for (int d = 0; d < D; ++d) {
				const int cc = origin[d] + ((q >> d) & 1);
				in = in && (0 <= cc) && (cc < g->gn[d]);
				idx += cc * mul;
				mul *= g->gn[d];
			}
			if (in) { e += static_cast<T>(c[q]) * x[idx]; }
		}
		e -= static_cast<T>(b);
		ss += e * e;
		any = true;
	}
};

template <int D, typename T>
__global__ __launch_bounds__(kThreads) void k_point_residual(EmitArgs a, long n, const float* __restrict__ pos,
                                                              const float* __restrict__ nrm, const float* __restrict__ base,
                                                              const float* __restrict__ val, const T* __restrict__ x,
                                                              float* __restrict__ r, uint32_t* __restrict__ keys, RobustRecord* rec)
{
	const long i = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x;
	float res = -1.0f;
	if (i < n) {
		const float bw    = a.has_pw ? base[i] : 1.0f;  // decides which rows exist; the coefficients take the weight 1
		const float value = a.has_val ? val[i] : 0.0f;
		RowResidual<D, T> acc{x, &a.g, a.invalid_key, T(0), false};
		point_rows<D>(a, i, pos, nrm, 1.0f, bw, value, acc);
		if (acc.any) { res = static_cast<float>(root(acc.ss)); }
		r[i] = res;
		if (keys) { keys[i] = res >= 0.0f ? __float_as_uint(res) : 0xFFFFFFFFu; }
	}
	const unsigned long long live = __ballot(res >= 0.0f);
	if ((threadIdx.x & 63) == 0 && live != 0) { atomicAdd(&rec->m, static_cast<unsigned int>(__popcll(live))); }
}

__global__ void k_pick_scale(RobustRecord* rec, const uint32_t* __restrict__ sorted, float user_scale)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) { return; }
	const unsigned int m = rec->m;
	float s = 0.0f;
	if (user_scale > 0.0f) {
		s = user_scale;
	} else if (m > 0) {
		s = 1.4826f * __uint_as_float(sorted[(m - 1) / 2]);
	}
	rec->scale = s;
}

__global__ __launch_bounds__(kThreads) void k_robust_weights(long n, const float* __restrict__ r, const float* __restrict__ base,
                                                              float* __restrict__ omega, float* __restrict__ pw, int loss, float c,
                                                              RobustRecord* rec)
{
	const float s = rec->scale;
	if (s == 0.0f) { return; }  // more than half of the points fit exactly: the step changes nothing
	const long i = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x;
	float change = 0.0f;
	bool  zero   = false;
	if (i < n) {
		const float ri = r[i];
		float w = 1.0f;
		if (!(ri < 0.0f)) {
			const float u = ri / (s * c);
			if (loss == FI_LOSS_HUBER) {
				w = u <= 1.0f ? 1.0f : 1.0f / u;
			} else if (loss == FI_LOSS_CAUCHY) {
				w = 1.0f / (1.0f + u * u);
			} else {
				const float t = 1.0f - u * u;
				w = u < 1.0f ? t * t : 0.0f;
			}
			zero = w == 0.0f;
		}
		change   = fabsf(w - omega[i]);
		omega[i] = w;
		pw[i]    = (base ? base[i] : 1.0f) * sqrtf(w);
	}
	for (int off = 32; off > 0; off >>= 1) { change = fmaxf(change, __shfl_xor(change, off)); }
	const unsigned long long zeros = __ballot(zero);
	if ((threadIdx.x & 63) == 0) {
		if (change > 0.0f) { atomicMax(&rec->dmax_bits, __float_as_uint(change)); }
		if (zeros != 0) { atomicAdd(&rec->zeroed, static_cast<unsigned int>(__popcll(zeros))); }
	}
}

__global__ __launch_bounds__(kThreads) void k_fill_ones(long n, float* __restrict__ out)
{
	const long i = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x;
	if (i < n) { out[i] = 1.0f; }
}

inline dim3 grid_for(long n) { return dim3(static_cast<unsigned int>((n + kThreads - 1) / kThreads)); }

// the caller's weights of a batch, as they were given: nullptr = every weight 1
const float* base_weights(const PointBatch* b)
{
	if (b->reweighted) { return b->had_pw ? b->pw0.as<float>() : nullptr; }
	return b->has_pw ? b->pw.as<float>() : nullptr;
}

// The field in the context's precision on the device: the last solution where it lives, the caller's device array, or a
// staged / widened copy in the context's robust.field
template <typename T>
const T* native_field(fi_ctx* c, const float* field, int memory)
{
	if (!field) {
		FI_REQUIRE(c->vectors_ready, FI_ERR_STATE, "no field given and no solution yet");
		return owned<T>(c, c->x);
	}
	const int64_t n = c->g.nown;
	if (sizeof(T) == sizeof(float)) {
		if (memory == FI_DEVICE) { return reinterpret_cast<const T*>(field); }
		c->robust.field.alloc(sizeof(float) * n);
		FI_HIP_TRY(hipMemcpyAsync(c->robust.field.p, field, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
		return c->robust.field.as<T>();
	}
	DevBuf       tmp;
	const float* src = field;
	if (memory == FI_HOST) {
		tmp.alloc(sizeof(float) * n);
		FI_HIP_TRY(hipMemcpyAsync(tmp.p, field, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
		src = tmp.as<float>();
	}
	c->robust.field.alloc(sizeof(T) * n);
	hipLaunchKernelGGL((k_from_float<T>), dim3(blocks_for(n)), dim3(kThreads), 0, c->stream, n, src, c->robust.field.as<T>());
	FI_HIP_TRY(hipGetLastError());
	FI_HIP_TRY(hipStreamSynchronize(c->stream));  // (before tmp goes)
	return c->robust.field.as<T>();
}

template <int D, typename T>
void residual_pass_dim(fi_ctx* c, const T* x, float* r, uint32_t* keys, RobustRecord* rec)
{
	long off = 0;
	for (const PointBatch* b : c->batches) {
		if (b->n <= 0 || b->prior) { continue; }
		const float* nrm  = b->has_nrm ? b->nrm.as<float>() : nullptr;
		const float* base = base_weights(b);
		EmitArgs a;
		a.g   = c->g;
		a.vw  = b->vw;
		a.gw  = b->gw;
		a.vk  = b->vk;
		a.gk  = b->gk;
		a.has_nrm = nrm != nullptr;
		a.has_pw  = base != nullptr;
		a.has_val = b->has_val;
		a.rows_per_point = (nrm != nullptr && b->gw != 0.0f) ? 1 + D : 1;  // as emit_point_rows decides
		a.invalid_key = static_cast<uint32_t>(static_cast<int64_t>(c->g.cn[0]) * c->g.cn[1] * c->g.cn[2]);
		a.pos_scale = 1.0f;
		a.nrm_scale = 1.0f;
		hipLaunchKernelGGL((k_point_residual<D, T>), grid_for(b->n), dim3(kThreads), 0, c->stream, a, b->n, b->pos.as<float>(), nrm, base,
		                   b->has_val ? b->val.as<float>() : nullptr, x, r + off, keys ? keys + off : nullptr, rec);
		FI_HIP_TRY(hipGetLastError());
		off += b->n;
	}
}

template <typename T>
void residual_pass(fi_ctx* c, const float* field, int memory, float* r, uint32_t* keys, RobustRecord* rec)
{
	const T* x = native_field<T>(c, field, memory);
	switch (c->g.ndim) {
	case 1: residual_pass_dim<1, T>(c, x, r, keys, rec); break;
	case 2: residual_pass_dim<2, T>(c, x, r, keys, rec); break;
	default: residual_pass_dim<3, T>(c, x, r, keys, rec); break;
	}
}

RobustRecord* fresh_record(fi_ctx* c)
{
	c->robust.rec.alloc(sizeof(RobustRecord));
	FI_HIP_TRY(hipMemsetAsync(c->robust.rec.p, 0, sizeof(RobustRecord), c->stream));
	return c->robust.rec.as<RobustRecord>();
}

// the row tables back to their pool, every batch emitted again: the path and the order of the first emission
void emit_again(fi_ctx* c)
{
	for (auto* pb : c->pending) { c->pending_pool.push_back(pb); }
	c->pending.clear();
	for (const PointBatch* b : c->batches) {
		emit_point_rows(c, b->n, b->pos.as<float>(), b->has_nrm ? b->nrm.as<float>() : nullptr, b->has_pw ? b->pw.as<float>() : nullptr,
		                b->has_val ? b->val.as<float>() : nullptr, b->vw, b->vk, b->gw, b->gk);
	}
	c->assembled = false;
}

}  // namespace

long robust_point_count(const fi_ctx* c)
{
	long n = 0;
	for (const PointBatch* b : c->batches) {
		if (b->n > 0 && !b->prior) { n += b->n; }
	}
	return n;
}

long robust_check(const fi_ctx* c)
{
	FI_REQUIRE(c->nranks == 1, FI_ERR_UNSUPPORTED, "robust fits on a slab context: a rank sees only its own points and the median is global");
	for (const PointBatch* b : c->batches) {
		FI_REQUIRE(!(b->n > 0 && b->has_nrm && b->gk == FI_GRADIENT_LINEAR_INTERPOLATION), FI_ERR_UNSUPPORTED,
		           "robust fits with FI_GRADIENT_LINEAR_INTERPOLATION: its rows live among the generic rows");
	}
	FI_REQUIRE(c->generic.nrows == 0 && c->generic.ntrip == 0, FI_ERR_UNSUPPORTED, "robust fits on a context that holds fi_add_rows_coo rows");
	const long n = robust_point_count(c);
	FI_REQUIRE(n > 0, FI_ERR_STATE, "no data points: call fi_add_points first");
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld data points", n);  // (one thread per point, 32-bit sort counts)
	return n;
}

void robust_residuals(fi_ctx* c, const float* field, float* residuals, int memory)
{
	const long n = robust_check(c);
	FI_REQUIRE(residuals != nullptr, FI_ERR_INVALID, "residuals is null");
	AllocStream alloc_on(c->stream);
	RobustRecord* rec = fresh_record(c);
	float* r = residuals;
	if (memory == FI_HOST) {
		c->robust.r.alloc(sizeof(float) * n);
		r = c->robust.r.as<float>();
	}
	c->dtype == FI_F64 ? residual_pass<double>(c, field, memory, r, nullptr, rec) : residual_pass<float>(c, field, memory, r, nullptr, rec);
	if (memory == FI_HOST) { FI_HIP_TRY(hipMemcpyAsync(residuals, r, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream)); }
	FI_HIP_TRY(hipStreamSynchronize(c->stream));
}

RobustStep robust_reweight(fi_ctx* c, const float* field, int loss, float tuning, float scale, float* omega, int memory)
{
	const long n = robust_check(c);
	FI_REQUIRE(loss == FI_LOSS_HUBER || loss == FI_LOSS_CAUCHY || loss == FI_LOSS_TUKEY, FI_ERR_INVALID, "unknown loss %d", loss);
	FI_REQUIRE(tuning >= 0.0f && tuning <= 3.0e38f, FI_ERR_INVALID, "tuning must be >= 0 (got %g)", static_cast<double>(tuning));  // (NaN fails)
	FI_REQUIRE(scale >= 0.0f && scale <= 3.0e38f, FI_ERR_INVALID, "scale must be >= 0 (got %g)", static_cast<double>(scale));
	const float c_tune = tuning > 0.0f ? tuning : (loss == FI_LOSS_HUBER ? 1.345f : loss == FI_LOSS_CAUCHY ? 2.385f : 4.685f);
	AllocStream  alloc_on(c->stream);
	RobustState& st = c->robust;
	hipStream_t  s  = c->stream;
	if (st.n != n) {  // no reweighting since the points changed: every omega is 1
		st.omega.alloc(sizeof(float) * n);
		hipLaunchKernelGGL(k_fill_ones, grid_for(n), dim3(kThreads), 0, s, n, st.omega.as<float>());
		FI_HIP_TRY(hipGetLastError());
		st.n = n;
	}
	st.r.alloc(sizeof(float) * n);
	st.keys.alloc(sizeof(uint32_t) * n);
	st.sorted.alloc(sizeof(uint32_t) * n);
	RobustRecord* rec = fresh_record(c);
	c->dtype == FI_F64 ? residual_pass<double>(c, field, memory, st.r.as<float>(), st.keys.as<uint32_t>(), rec)
	                   : residual_pass<float>(c, field, memory, st.r.as<float>(), st.keys.as<uint32_t>(), rec);
	if (!(scale > 0.0f)) {
		size_t bytes = 0;
		FI_HIP_TRY(sort_keys_u32(nullptr, bytes, st.keys.as<uint32_t>(), st.sorted.as<uint32_t>(), static_cast<unsigned int>(n), s));
		st.tmp.alloc(bytes);
		FI_HIP_TRY(sort_keys_u32(st.tmp.p, bytes, st.keys.as<uint32_t>(), st.sorted.as<uint32_t>(), static_cast<unsigned int>(n), s));
	}
	hipLaunchKernelGGL(k_pick_scale, dim3(1), dim3(64), 0, s, rec, st.sorted.as<uint32_t>(), scale);
	FI_HIP_TRY(hipGetLastError());
	// base stays in the batch (pw0), the new weights go where every emission reads them (pw)
	long off = 0;
	for (PointBatch* b : c->batches) {
		if (b->n <= 0 || b->prior) { continue; }
		if (!b->reweighted) {
			b->had_pw = b->has_pw;
			if (b->had_pw) {
				b->pw0.alloc(sizeof(float) * b->n);
				FI_HIP_TRY(hipMemcpyAsync(b->pw0.p, b->pw.p, sizeof(float) * b->n, hipMemcpyDeviceToDevice, s));
			} else {
				b->pw.alloc(sizeof(float) * b->n);
				hipLaunchKernelGGL(k_fill_ones, grid_for(b->n), dim3(kThreads), 0, s, b->n, b->pw.as<float>());
				FI_HIP_TRY(hipGetLastError());
				b->has_pw = true;
			}
			b->reweighted = true;
		}
		hipLaunchKernelGGL(k_robust_weights, grid_for(b->n), dim3(kThreads), 0, s, b->n, st.r.as<float>() + off, base_weights(b),
		                   st.omega.as<float>() + off, b->pw.as<float>(), loss, c_tune, rec);
		FI_HIP_TRY(hipGetLastError());
		off += b->n;
	}
	RobustRecord* h = static_cast<RobustRecord*>(pinned(c, 0, sizeof(RobustRecord)));
	FI_HIP_TRY(hipMemcpyAsync(h, rec, sizeof(RobustRecord), hipMemcpyDeviceToHost, s));
	if (omega) {
		FI_HIP_TRY(hipMemcpyAsync(omega, st.omega.p, sizeof(float) * n, memory == FI_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
	}
	FI_HIP_TRY(hipStreamSynchronize(s));
	RobustStep out;
	out.scale         = h->scale;
	out.points_used   = h->m;
	out.points_zeroed = h->zeroed;
	std::memcpy(&out.max_weight_change, &h->dmax_bits, sizeof(float));
	if (out.scale != 0.0f) {
		emit_again(c);
		FI_HIP_TRY(hipStreamSynchronize(s));
	}
	return out;
}

void robust_reset(fi_ctx* c)
{
	bool any = false;
	for (PointBatch* b : c->batches) {
		if (!b->reweighted) { continue; }
		if (b->had_pw) {
			FI_HIP_TRY(hipMemcpyAsync(b->pw.p, b->pw0.p, sizeof(float) * b->n, hipMemcpyDeviceToDevice, c->stream));
		} else {
			b->has_pw = false;
		}
		b->reweighted = false;
		any = true;
	}
	c->robust.n = 0;
	if (!any) { return; }
	AllocStream alloc_on(c->stream);
	emit_again(c);
	FI_HIP_TRY(hipStreamSynchronize(c->stream));
}

}  // namespace fi
