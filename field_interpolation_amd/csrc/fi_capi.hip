// fi_capi.hip -- the C ABI of include/fi_hip.h (every entry point cites the reference interface it replaces there): contexts,
// model, points, assemble, the solver entry points and their options, statistics.  Nothing throws or aborts across it.
#include "fi_solver_internal.h"
#include "fi_stage.h"
#include "fi_workers.h"
#include "fi_iso.h"
#include "fi_dual.h"
#include "fi_sample.h"
#include "fi_nearest.h"
#include "fi_knn.h"
#include "fi_orient.h"
#include "fi_surface.h"
#include "fi_ray.h"
#include "fi_robust.h"
#include "fi_parts.h"
#include "fi_simplify.h"
#include "fi_smooth.h"
#include "fi_meshpts.h"
#include "fi_register.h"
#include "fi_cloud.h"
#include "fi_cluster.h"
#include "fi_plane.h"
#include "fi_shape.h"
#include "fi_align.h"
#include "fi_mls.h"
#include "fi_feature.h"
#include "fi_depth.h"
#include "fi_march.h"
#include "fi_colour.h"

#include <memory>

namespace fi {

// ------------------------------------------------------------------------------------------------
static thread_local std::string g_error;

void set_error(const char* fmt, ...)
{
	char    buf[1024];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	g_error = buf;
}


// upscale_field (field_interpolation.cpp:431-485): one thread per point of the large lattice.
namespace {
struct UpscaleArgs {
	int ndim;
	int ssz[3], lsz[3];
};
__global__ __launch_bounds__(kThreads) void k_upscale(UpscaleArgs a, int64_t nlarge, const float* __restrict__ small,
                                                       float* __restrict__ out)
{
	const int64_t li = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
	if (li >= nlarge) { return; }
	int     base[3];
	float   t[3];
	int64_t rest = li;
	for (int d = 0; d < a.ndim; ++d) {
		const int c = static_cast<int>(rest % a.lsz[d]);
		rest /= a.lsz[d];
		const float sp = static_cast<float>(c) * (static_cast<float>(a.ssz[d]) - 1.0f) /
		                 (static_cast<float>(a.lsz[d]) - 1.0f);
		// a large axis of ONE point: 0 * (small - 1) / 0 is NaN.  The reference, as compiled for x86, floors it to INT_MIN, keeps
		// no sample and writes 0 (:477-478); here the cast would give 0 and NaN weights, so the point is sent far outside.
		const bool  ok = sp == sp;
		const float fl = floorf(sp);
		base[d] = ok ? static_cast<int>(fl) : -4;
		t[d]    = ok ? sp - static_cast<float>(base[d]) : 0.0f;
	}
	float wsum = 0.0f, fsum = 0.0f;
	for (int q = 0; q < (1 << a.ndim); ++q) {
		int64_t idx = 0, stride = 1;
		float   w  = 1.0f;
		bool    in = true;
		for (int d = 0; d < a.ndim; ++d) {
			const int up = (q >> d) & 1;
			const int cc = base[d] + up;
			idx += stride * cc;
			stride *= a.ssz[d];
			w *= up ? t[d] : 1.0f - t[d];
			in = in && (0 <= cc) && (cc < a.ssz[d]);
		}
		if (in) {
			wsum += w;
			fsum += w * small[idx];
		}
	}
	out[li] = (wsum == 0.0f) ? 0.0f : fsum / wsum;
}

// ---- whole fields and handles of their own (the *_field and *_destroy entry points) ----
// the points of a lattice; every size at least 1
int64_t lattice_points(int ndim, const int* sizes)
{
	int64_t n = 1;
	for (int d = 0; d < ndim; ++d) {
		FI_REQUIRE(sizes[d] >= 1, FI_ERR_INVALID, "sizes[%d] = %d", d, sizes[d]);
		n *= sizes[d];
	}
	return n;
}

// fi_mesh_destroy / fi_points_destroy / fi_surface_destroy: the object's buffers go back on the device it lives on
template <typename Handle>
int destroy_handle(Handle* h)
{
	if (!h) { return FI_OK; }
	int dev = 0;
	const bool switched = hipGetDevice(&dev) == hipSuccess && dev != h->device && hipSetDevice(h->device) == hipSuccess;
	delete h;
	if (switched) { (void)hipSetDevice(dev); }
	return FI_OK;
}

}  // namespace

void check_ctx(const fi_ctx* c) { FI_REQUIRE(c != nullptr, FI_ERR_INVALID, "null context"); }

void check_assembled(const fi_ctx* c)
{
	check_ctx(c);
	FI_REQUIRE(c->assembled, FI_ERR_STATE, "fi_assemble has not been called");
}

void bind_device(const fi_ctx* c) { FI_HIP_TRY(hipSetDevice(c->device)); }

fi_ctx* create_ctx(int ndim, const int* sizes, int dtype, int rank, int nranks)
{
	FI_REQUIRE(1 <= ndim && ndim <= FI_MAX_DIM, FI_ERR_INVALID, "ndim must be 1..%d (got %d)", FI_MAX_DIM, ndim);
	FI_REQUIRE(sizes != nullptr, FI_ERR_INVALID, "sizes is null");
	FI_REQUIRE(dtype == FI_F32 || dtype == FI_F64, FI_ERR_INVALID, "unknown dtype %d", dtype);
	FI_REQUIRE(nranks >= 1 && 0 <= rank && rank < nranks, FI_ERR_INVALID, "bad rank %d of %d", rank, nranks);
	int64_t n = 1;
	for (int d = 0; d < ndim; ++d) {
		FI_REQUIRE(sizes[d] >= 1, FI_ERR_INVALID, "sizes[%d] = %d", d, sizes[d]);
		n *= sizes[d];
		FI_REQUIRE(static_cast<int64_t>(sizes[d]) + 1 < (1 << 20), FI_ERR_INVALID, "sizes[%d] too large", d);
	}
	FI_REQUIRE(n < (1LL << 31), FI_ERR_UNSUPPORTED, "lattice has %lld unknowns; the reference indexes with int",
	           static_cast<long long>(n));
	FI_REQUIRE(nranks == 1 || sizes[ndim - 1] >= nranks, FI_ERR_INVALID, "fewer planes (%d) than ranks (%d)",
	           sizes[ndim - 1], nranks);
	auto* c = new fi_ctx();
	try {
		c->dtype  = dtype;
		c->rank   = rank;
		c->nranks = nranks;
		FI_HIP_TRY(hipGetDevice(&c->device));
		c->stream = stream_take();
		c->halo = 1;
		c->stats.field_estimate = -1.0;  // (fi_stats: no solve yet, and none by the field)
		compute_geom(c, ndim, sizes);
		c->scal.alloc(3 * sizeof(CgScalars));  // [0]: the state every kernel and the host look at, [1]: mid-iteration copy,
		                                       // [2]: landing place of the dot products summed over slabs (rank sets)
		FI_HIP_TRY(hipMemset(c->scal.p, 0, 2 * sizeof(CgScalars)));
		c->scal_host = static_cast<CgScalars*>(pinned_take(sizeof(CgScalars), &c->scal_host_cap));
		// default Weights (field_interpolation.hpp:75-95)
		c->w = fi_weights{1.0f, 1.0f, 0.0f, 0.0f, 0.5f, 0.0f, 0.0f, 0.0f, FI_VALUE_LINEAR_INTERPOLATION,
		                  FI_GRADIENT_CELL_EDGES};
	} catch (...) {
		fi_ctx_destroy(c);
		throw;
	}
	return c;
}


}  // namespace fi

// ===================================================================================================
// C ABI

extern "C" {

const char* fi_last_error(void) { return fi::g_error.c_str(); }

int fi_device_count(int* count)
{
	FI_API_BEGIN
	FI_REQUIRE(count != nullptr, FI_ERR_INVALID, "count is null");
	int n = 0;
	const hipError_t e = hipGetDeviceCount(&n);
	*count = (e == hipSuccess) ? n : 0;
	FI_API_END
}

int fi_ctx_create(fi_ctx** out, int ndim, const int* sizes, int dtype)
{
	FI_API_BEGIN
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "out is null");
	*out = fi::create_ctx(ndim, sizes, dtype, 0, 1);
	FI_API_END
}

int fi_ctx_create_slab(fi_ctx** out, int ndim, const int* sizes, int dtype, int rank, int nranks)
{
	FI_API_BEGIN
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "out is null");
	*out = fi::create_ctx(ndim, sizes, dtype, rank, nranks);
	FI_API_END
}

int fi_ctx_destroy(fi_ctx* c)
{
	if (!c) { return FI_OK; }
	(void)hipSetDevice(c->device);
	// The context's blocks go to the pool of fi_pool.hip: nothing in flight may still touch them.  Everything that works on
	// a context's blocks is enqueued on one of ITS streams (the solver stream -- a group's members share member 0's --, the
	// helper streams of the assembly, the communication stream): those are drained, level by level as the recursion below
	// reaches them; the rest of the device (other contexts, torch, other threads) is not stalled.
	bool drained = true;
	for (hipStream_t st : {c->stream, c->level_stream, c->level_stream2, c->build_stream, c->comm_stream}) {
		if (st && hipStreamSynchronize(st) != hipSuccess) { drained = false; }
	}
	struct Quiescent {
		bool was;
		explicit Quiescent(bool ok) : was(fi::pool_quiescent) { fi::pool_quiescent = ok; }
		~Quiescent() { fi::pool_quiescent = was; }
	} quiescent(drained);
	for (auto* pb : c->pending) { delete pb; }
	for (auto* pb : c->pending_pool) { delete pb; }
	for (auto* b : c->batches) { delete b; }
	for (auto* b : c->batches_pool) { delete b; }
	if (c->coarse) { fi_ctx_destroy(c->coarse); }
	if (c->twin) { fi_ctx_destroy(c->twin); }
	c->pending.clear();
	c->pending_pool.clear();
	for (auto e : c->ev) { (void)hipEventDestroy(e); }
	for (auto e : c->ev_prec) { (void)hipEventDestroy(e); }
	fi::stream_give(c->level_stream, drained);
	if (c->ev_level) { (void)hipEventDestroy(c->ev_level); }
	fi::stream_give(c->level_stream2, drained);
	if (c->build_stream) {
		fi::stream_give(c->build_stream, drained);
		(void)hipEventDestroy(c->ev_build);
	}
	if (c->ev_level2) { (void)hipEventDestroy(c->ev_level2); }
	if (c->comm_stream) {
		fi::stream_give(c->comm_stream, drained);
		(void)hipEventDestroy(c->ev_ready);
		(void)hipEventDestroy(c->ev_halo);
	}
	if (c->comm && c->owns_comm) { fi::comm_destroy(c->comm); }
	// pinned blocks go back to the pool only when nothing can still be copying into or out of them (the stop-flag copies of an
	// unwatched level, point staging): a context whose streams did not drain frees them instead -- hipHostFree waits
	if (c->scal_host) {
		if (drained) { fi::pinned_give(c->scal_host, c->scal_host_cap); } else { (void)hipHostFree(c->scal_host); }
	}
	for (int s = 0; s < 3; ++s) {
		if (!c->pin[s]) { continue; }
		if (drained) { fi::pinned_give(c->pin[s], c->pin_bytes[s]); } else { (void)hipHostFree(c->pin[s]); }
	}
	if (c->ev_unwatched) { (void)hipEventDestroy(c->ev_unwatched); }
	if (c->ev_asm0) {
		(void)hipEventDestroy(c->ev_asm0);
		(void)hipEventDestroy(c->ev_asm1);
	}
	if (c->stream && c->owns_stream) { fi::stream_give(c->stream, drained); }
	fi::nearest_release(c);
	delete c;
	return FI_OK;
}

int fi_memory_pool(long long keep_bytes, long long* cached_bytes)
{
	FI_API_BEGIN
	const size_t keep = keep_bytes < 0 ? ~size_t(0) : static_cast<size_t>(keep_bytes);
	const size_t left = fi::pool_trim(keep);
	if (keep == 0) {  // "nothing left over from earlier contexts": neither their blocks nor what they learnt
		fi::forget_iterations();
		fi::forget_lambdas();
	}
	if (cached_bytes) { *cached_bytes = static_cast<long long>(left); }
	FI_API_END
}

int fi_slab_partition(int planes, int rank, int nranks, int* lo, int* hi)
{
	FI_API_BEGIN
	FI_REQUIRE(nranks >= 1 && 0 <= rank && rank < nranks && planes >= 0, FI_ERR_INVALID, "bad slab request");
	if (lo) { *lo = static_cast<int>(static_cast<int64_t>(rank) * planes / nranks); }
	if (hi) { *hi = static_cast<int>(static_cast<int64_t>(rank + 1) * planes / nranks); }
	FI_API_END
}

int fi_halo_width(const fi_weights* w, int* width)
{
	FI_API_BEGIN
	FI_REQUIRE(w && width, FI_ERR_INVALID, "null argument");
	const int reach = fi::model_reach(*w);
	*width = reach > 1 ? reach : 1;
	FI_API_END
}

int fi_slab_range(const fi_ctx* c, int* lo, int* hi)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	if (lo) { *lo = c->slab_lo; }
	if (hi) { *hi = c->slab_hi; }
	FI_API_END
}

int fi_slab_point_range(const fi_ctx* c, float* lo, float* hi)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	// Level l halves the lattice l times (coarse plane k sits on fine plane k * 2^l; this rank keeps coarse planes
	// ceil(slab_lo / 2^l) .. ceil(slab_hi / 2^l) - 1), and a rank needs every cell that touches an owned plane of
	// that level plus one cell of margin for the nearest-neighbour kernels: 2 cells of 2^l fine planes below, 1 above --
	// 2 above as well, because a level halved cell-centred (fi_ctx::cc) sees a point up to half a coarse cell further down
	// (position / 2^l - (1 - 2^-l) / 2).
	// A hierarchy whose deeper levels are replicated (whole lattices on every rank once the slabs would be thinner than 4
	// planes: build_levels) is assembled from ALL the points: the range is then everything.
	const int L = c->levels_wanted > 0 ? c->levels_wanted : 0;
	int first_tail = 0;
	const int nlevels = fi::plan_levels(c, &first_tail);
	if (c->nranks > 1 && first_tail <= nlevels) {
		if (lo) { *lo = -std::numeric_limits<float>::max(); }
		if (hi) { *hi = std::numeric_limits<float>::max(); }
		return FI_OK;
	}
	const float cell = static_cast<float>(1 << (L < 20 ? L : 20));
	if (lo) { *lo = static_cast<float>(c->slab_lo) - 2.0f * cell; }
	if (hi) { *hi = static_cast<float>(c->slab_hi) + (L > 0 ? 2.0f : 1.0f) * cell; }
	FI_API_END
}

int fi_set_model(fi_ctx* c, const fi_weights* w)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	FI_REQUIRE(w != nullptr, FI_ERR_INVALID, "weights is null");
	c->w         = *w;
	c->model_set = true;
	c->assembled = false;
	for (fi_ctx* l = c; l; l = l->coarse) { l->poly_lambda = 0; }  // the polynomial preconditioner's bound belongs to the model
	if (c->twin) {
		for (fi_ctx* l = c->twin; l; l = l->coarse) { l->poly_lambda = 0; }
	}
	FI_API_END
}

int fi_add_points(fi_ctx* c, long n, const float* positions, const float* normals, const float* point_weights,
                  const float* values, float value_weight, int value_kernel, float gradient_weight, int gradient_kernel,
                  int memory)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	fi::bind_device(c);
	FI_REQUIRE(n >= 0, FI_ERR_INVALID, "negative point count");
	if (n == 0) { return FI_OK; }
	FI_REQUIRE(positions != nullptr, FI_ERR_INVALID, "positions is null");  // CHECK_NOTNULL_F, cpp:382
	FI_REQUIRE(value_kernel == FI_VALUE_NEAREST_NEIGHBOR || value_kernel == FI_VALUE_LINEAR_INTERPOLATION,
	           FI_ERR_INVALID, "Unknown value kernel: %d", value_kernel);
	FI_REQUIRE(!(value_kernel == FI_VALUE_NEAREST_NEIGHBOR && normals == nullptr), FI_ERR_INVALID,
	           "nearest-neighbour value kernel needs normals (field_interpolation.cpp:361)");
	if (normals) {
		FI_REQUIRE(gradient_kernel >= 0 && gradient_kernel <= 2, FI_ERR_INVALID, "Unknown gradient kernel: %d",
		           gradient_kernel);  // ABORT_F, cpp:238
// (GradientKernel::kLinearInterpolation over slabs: its rows are kept as triplets with local columns, fi_generic.hip)
	}
	fi::check_memory(memory);
	const int D = c->g.ndim;
	fi::DevBuf dpos, dnrm, dpw, dval;
	const float *p = positions, *g = normals, *w = point_weights, *v = values;
	if (memory == FI_HOST) {
		auto up = [&](fi::DevBuf& b, const float* src, size_t count) -> const float* {
			if (!src) { return nullptr; }
			b.alloc(sizeof(float) * count);
			FI_HIP_TRY(hipMemcpyAsync(b.p, src, sizeof(float) * count, hipMemcpyHostToDevice, c->stream));
			return b.as<float>();
		};
		p = up(dpos, positions, static_cast<size_t>(n) * D);
		g = up(dnrm, normals, static_cast<size_t>(n) * D);
		w = up(dpw, point_weights, static_cast<size_t>(n));
		v = up(dval, values, static_cast<size_t>(n));
	}
	fi::nearest_release(c);  // (a new point set)
	fi::add_points_device(c, n, p, g, w, v, value_weight, value_kernel, gradient_weight, gradient_kernel);
	c->assembled = false;
	FI_API_END
}

}  // extern "C"

namespace fi {
// positions / normals / weights / values already on the device
void add_points_device(fi_ctx* c, long n, const float* p, const float* g, const float* w, const float* v, float value_weight,
                       int value_kernel, float gradient_weight, int gradient_kernel)
{
	const int D = c->g.ndim;
	{   // keep the points on the device: coarser levels of a multilevel solve are assembled from them
		fi::PointBatch* b = nullptr;
		if (!c->batches_pool.empty()) {
			b = c->batches_pool.back();
			c->batches_pool.pop_back();
		} else {
			b = new fi::PointBatch();
		}
		c->batches.push_back(b);
		auto keep = [&](fi::DevBuf& dst, const float* src, size_t count) {
			if (!src) { return false; }
			dst.alloc(sizeof(float) * count);
			FI_HIP_TRY(hipMemcpyAsync(dst.p, src, sizeof(float) * count, hipMemcpyDeviceToDevice, c->stream));
			return true;
		};
		b->n = n;
		b->prior = false;
		b->reweighted = false;  // (a new batch carries the caller's weights; the robust factors start again from 1)
		b->had_pw     = false;
		c->robust.n   = 0;
		keep(b->pos, p, static_cast<size_t>(n) * D);
		b->has_nrm = keep(b->nrm, g, static_cast<size_t>(n) * D);
		b->has_pw  = keep(b->pw, w, static_cast<size_t>(n));
		b->has_val = keep(b->val, v, static_cast<size_t>(n));
		b->vw = value_weight;
		b->gw = gradient_weight;
		b->vk = value_kernel;
		b->gk = gradient_kernel;
	}
	const bool lin = g && gradient_kernel == FI_GRADIENT_LINEAR_INTERPOLATION;
	// cell-local rows (value rows; gradient rows of the nearest-neighbour / cell-edge kernels) ...
	fi::emit_point_rows(c, n, p, g, w, v, value_weight, value_kernel, lin ? 0.0f : gradient_weight,
	                    lin ? FI_GRADIENT_CELL_EDGES : gradient_kernel);
	// ... and the 3-point-wide rows of GradientKernel::kLinearInterpolation as generic sparse rows
	if (lin && gradient_weight != 0.0f) { fi::generic_add_gradient_linear(c, n, p, g, w, gradient_weight); }
	FI_HIP_TRY(hipStreamSynchronize(c->stream));
}
}  // namespace fi

extern "C" {

int fi_add_border_prior(fi_ctx* c, float weight)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	fi::bind_device(c);
	if (weight == 0.0f) { return FI_OK; }  // add_equation skips zero weights (sparse_linear.cpp:36)
	// The distance is to the nearest point of the WHOLE cloud (sdf_field.cpp:218-246); a slab context holds only the points
	// of fi_slab_point_range, so the prior of a decomposed lattice would be silently wrong (or infinite on a rank without
	// points): not supported -- add the prior's rows with fi_add_points(FI_VALUE_NEAREST_NEIGHBOR) from the caller's side.
	FI_REQUIRE(c->nranks == 1, FI_ERR_UNSUPPORTED, "fi_add_border_prior on a slab context: a rank sees only its own points");
	bool any = false;
	for (const fi::PointBatch* b : c->batches) { any = any || (b->n > 0 && !b->prior); }
	FI_REQUIRE(any, FI_ERR_STATE, "fi_add_border_prior needs the data points: call it after fi_add_points");
	fi::DevBuf pos, val, zero;
	const int64_t nb = fi::border_prior_points(c, pos, val);
	if (nb > 0) {
		zero.alloc(sizeof(float) * nb * c->g.ndim);
		FI_HIP_TRY(hipMemsetAsync(zero.p, 0, sizeof(float) * nb * c->g.ndim, c->stream));
		// the row [1] * w, rhs d * w at the lattice point itself: a nearest-neighbour value constraint with a zero gradient
		fi::add_points_device(c, static_cast<long>(nb), pos.as<float>(), zero.as<float>(), nullptr, val.as<float>(), weight,
		                      FI_VALUE_NEAREST_NEIGHBOR, 0.0f, FI_GRADIENT_NEAREST_NEIGHBOR);
		c->batches.back()->prior = true;
	}
	c->assembled = false;
	FI_API_END
}

int fi_add_rows_coo(fi_ctx* c, long nrows, long ntriplets, const fi_triplet* triplets, const float* rhs, int memory)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	fi::bind_device(c);
	FI_REQUIRE(nrows >= 0 && ntriplets >= 0, FI_ERR_INVALID, "negative count");
	fi::check_memory(memory);
	FI_REQUIRE(c->nranks == 1, FI_ERR_UNSUPPORTED, "generic rows need an undivided lattice");
	FI_REQUIRE((ntriplets == 0 || triplets) && (nrows == 0 || rhs), FI_ERR_INVALID, "null buffer");
	fi::generic_add_coo(c, nrows, ntriplets, triplets, rhs, memory);
	c->assembled = false;
	FI_API_END
}

int fi_clear_points(fi_ctx* c)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	for (auto* pb : c->pending) { c->pending_pool.push_back(pb); }  // keep the HBM buffers for the next batch
	c->pending.clear();
	for (auto* b : c->batches) { c->batches_pool.push_back(b); }
	c->batches.clear();
	c->robust.n = 0;
	fi::nearest_release(c);
	fi::generic_clear(c);
	c->assembled = false;
	FI_API_END
}

namespace fi {
// the time of the last fi_assemble, once its second event has passed (waits for it: the events are on the context's stream)
void finish_assemble_timing(fi_ctx* c)
{
	if (!c->asm_time_pending) { return; }
	c->asm_time_pending = false;
	if (hipEventSynchronize(c->ev_asm1) != hipSuccess) { return; }
	float ms = 0;
	if (hipEventElapsedTime(&ms, c->ev_asm0, c->ev_asm1) == hipSuccess) { c->stats.assemble_ms = ms; }
}
}  // namespace fi

int fi_assemble(fi_ctx* c)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	fi::bind_device(c);
	// The assembly is timed between two events of the context and nobody waits for the second one here: the caller's next
	// call -- normally the solve -- queues behind the assembly's last kernels instead of finding an idle GPU after a host
	// round trip (~0.1 ms of a config-4 step).  fi_get_stats (and the next fi_assemble) read the time.
	fi::finish_assemble_timing(c);
	if (!c->ev_asm0) {
		FI_HIP_TRY(hipEventCreate(&c->ev_asm0));
		FI_HIP_TRY(hipEventCreate(&c->ev_asm1));
	}
	const hipEvent_t e0 = c->ev_asm0, e1 = c->ev_asm1;
	fi::chain_mark(nullptr);
	FI_HIP_TRY(hipEventRecord(e0, c->stream));
	// Ghost planes along the decomposed axis.  reach: the widest model stencil, at least the cell reach (1) -- the width of
	// an exchange.  halo (planes stored): the reach, or the polynomial preconditioner's DEEP exchange: 2 (d - 1) planes of
	// r travel once per polynomial and the steps run redundantly on the shrinking ghost zone (cg_run_poly) instead of one
	// exchange per step -- 3-D lattices, 3 to 5 terms set before the assemble, slabs at least that thick on every rank.
	// Data facts every rank must see alike (fi_ctx::any_trip): one all-reduce in front of everything they decide
	{
		bool trip = c->generic.ntrip != 0, grad = !fi::holds_value_rows_only(c);
		if (c->facts_forced) {  // a loop-back group has looked at all its members
			trip = c->forced_trip;
			grad = c->forced_grad;
		} else if (c->nranks > 1 && fi::comm_ready(c)) {
			double* slot = (c->scal.as<fi::CgScalars>() + 2)->sums;
			double  v[2] = {trip ? 1.0 : 0.0, grad ? 1.0 : 0.0};
			FI_HIP_TRY(hipMemcpyAsync(slot, v, sizeof(v), hipMemcpyHostToDevice, c->stream));
			fi::allreduce_sum(c, slot, 2);
			FI_HIP_TRY(hipMemcpyAsync(v, slot, sizeof(v), hipMemcpyDeviceToHost, c->stream));
			FI_HIP_TRY(hipStreamSynchronize(c->stream));
			trip = v[0] > 0.0;
			grad = v[1] > 0.0;
		}
		c->any_trip        = trip;
		c->value_rows_only = !grad && !trip;
		c->facts_forced    = false;  // (the group's verdict is for THIS assemble: a later fi_assemble of a member looks again)
	}
	const int reach = fi::model_reach(c->w);
	const int want_reach = reach > 1 ? reach : 1;
	int want_halo = want_reach;
	if (c->nranks > 1 && c->g.ndim == 3 && c->poly_terms >= 3 && c->poly_terms <= 5 && !c->any_trip &&
	    !fi::test_switch("FI_NO_DEEP_HALO")) {
		const int deep = 2 * (c->poly_terms - 1);
		const int thinnest = c->g.gn[2] / c->nranks;  // (the equal split: floor(G / n) is the thinnest slab)
		if (deep > want_halo && thinnest >= deep) { want_halo = deep; }
	}
	// ... and the V-cycle's polynomial smoother (fp32 levels of value rows, 3 to 5 terms: poly_chain, fi_multigrid.hip)
	if (c->nranks > 1 && c->g.ndim == 3 && c->mg_mode == 1 && c->mg_smoother == 1 && c->levels_wanted > 0 && c->value_rows_only &&
	    !c->any_trip && (c->dtype == FI_F32 || c->mixed) && c->mg_terms >= 3 && c->mg_terms <= 5 &&
	    !(c->w.model_3 > 0 || c->w.model_4 > 0 || c->w.gradient_smoothness > 0) && !fi::test_switch("FI_NO_DEEP_HALO") &&
	    !fi::test_switch("FI_MG_FULL_SMOOTHER")) {
		const int deep = 2 * (c->mg_terms - 1);
		const int thinnest = c->g.gn[2] / c->nranks;
		if (deep > want_halo && thinnest >= deep) { want_halo = deep; }
	}
	c->min_slab = c->nranks > 1 ? c->g.gn[c->g.ndim - 1] / c->nranks : c->g.gn[c->g.ndim - 1];
	if (c->nranks > 1 && (want_halo != c->halo || want_reach != c->reach)) {
		c->halo  = want_halo;
		c->reach = want_reach;
		int sizes[3] = {c->g.gn[0], c->g.gn[1], c->g.gn[2]};
		fi::compute_geom(c, c->g.ndim, sizes);
		c->vectors_ready = false;
		c->vectors_stale = true;
	}
	if (c->nranks > 1) {
		FI_REQUIRE(c->slab_hi - c->slab_lo >= c->reach, FI_ERR_UNSUPPORTED,
		           "slab of %d planes is thinner than the stencil reach %d", c->slab_hi - c->slab_lo, c->reach);
	}
	// The coarser levels are problems of their own, assembled from the same point batches: a helper thread builds them on
	// a second stream while this one assembles the finest level (both are chains of small launches with host round trips
	// for list sizes; 256^3 with one coarser level: 2.05 -> 1.6 ms).  Contexts without triplet rows; the
	// helper's failure is re-raised here.  The helper does no communication: over slabs the levels' exchange of the
	// diagonal's ghost planes is done below, by this thread.
	// Mixed precision: the fp32 replica and ITS levels are the helper's work (the fp64 context keeps no levels of its own).
	const bool mixed64 = c->mixed && c->dtype == FI_F64;
	c->want_lump = mixed64 && fi::lumped_twin_wanted(c);  // (the assembly forms the replica's diagonal beside A^T b)
	const bool beside = (c->levels_wanted > 0 || mixed64) && !c->any_trip && !fi::test_switch("FI_SERIAL_LEVELS");
	if (beside && mixed64) {  // (levels an earlier, unmixed assemble may have left on this context)
		const int keep = c->levels_wanted;
		c->levels_wanted = 0;
		fi::build_levels(c);
		c->levels_wanted = keep;
	}
	if (beside) {
		if (!c->level_stream) {
			c->level_stream = fi::stream_take();
			FI_HIP_TRY(hipEventCreateWithFlags(&c->ev_level, hipEventDisableTiming));
		}
		FI_HIP_TRY(hipEventRecord(c->ev_level, c->stream));  // the point batches were written on the solver stream
		FI_HIP_TRY(hipStreamWaitEvent(c->level_stream, c->ev_level, 0));
		int         helper_code = FI_OK;
		std::string helper_msg;
		// mixed precision: the replica's finest level on `level_stream`, its coarser levels on `level_stream2` -- two more
		// chains of small launches beside this thread's (256^3, 3 coarser levels: 4.9 ms one after the other, 4.3 with one
		// helper, 3 with two)
		if (mixed64) {
			fi::twin_prepare(c);
			if (!c->level_stream2) {
				c->level_stream2 = fi::stream_take();
				FI_HIP_TRY(hipEventCreateWithFlags(&c->ev_level2, hipEventDisableTiming));
			}
			FI_HIP_TRY(hipStreamWaitEvent(c->level_stream2, c->ev_level, 0));
		}
		auto guarded = [&](auto&& work, int* code, std::string* msg) {
			try {
				FI_HIP_TRY(hipSetDevice(c->device));
				fi::AllocStream none(nullptr);  // (a helper's buffers: each level names its own stream, fi_levels.hip)
				work();
			} catch (const fi::Fail& f) {
				*code = f.code;
				*msg  = fi_last_error();  // thread-local: carried over to the caller's thread below
			} catch (...) {
				*code = FI_ERR_HIP;
				*msg  = "unexpected exception while building the coarser levels";
			}
		};
		const bool lumped = mixed64 && c->twin && c->twin->lumped;
		auto build = [&]() {
			guarded([&]() {
				if (lumped) {
					// (the replica's finest level needs the assembled fp64 operator: built below, by this thread)
				} else if (mixed64) {
					fi::twin_assemble(c, c->level_stream);
				} else {
					fi::build_levels(c, nullptr, c->level_stream);
				}
			}, &helper_code, &helper_msg);
		};
		int         helper2_code = FI_OK;
		std::string helper2_msg;
		auto build2 = [&]() {
			guarded([&]() { fi::build_levels(c->twin, c, c->level_stream2); }, &helper2_code, &helper2_msg);
		};
		// (persistent threads: fi_workers.h)
		fi::Worker *helper = nullptr, *helper2 = nullptr;
		try {
			if (!lumped) {
				helper = fi::worker_pool().acquire();
				helper->run(build);
			}
			if (mixed64) {
				helper2 = fi::worker_pool().acquire();
				helper2->run(build2);
			}
		} catch (...) {  // no thread to be had: the levels are built below, after the finest level, on their stream
		}
		int main_code = FI_OK;
		c->defer_scaling_exchange = true;  // slabs: the one exchange of the assembly comes after the ranks have agreed (below)
		try {
			fi::AllocStream alloc_on(c->stream);  // (this chain's buffers are first used on the solver stream: fi_internal.h)
			fi::chain_mark("threads started");
			fi::assemble(c);
			fi::chain_mark("finest: rows assembled");
			fi::generic_assemble(c);
			fi::stencil_prepare(c);
			fi::chain_mark("finest: stencil prepared");
			fi::operator_prepare(c);
			fi::chain_mark("finest: operator prepared");
		} catch (const fi::Fail& f) {
			main_code = f.code;
		} catch (...) {  // never leave the helper unjoined
			main_code = FI_ERR_HIP;
			fi::set_error("unexpected exception while assembling the finest level");
		}
		// The lumped replica needs nothing but the finest level this thread has just assembled: built here, on the solver
		// stream, while the helpers are still busy with the coarser levels (0.3 ms of a 256^3 assemble).  No communication
		// (its share of the assembly's one exchange comes with operator_finish_ghosts below).
		if (lumped && main_code == FI_OK) {
			try {
				fi::AllocStream alloc_on(c->stream);
				c->twin->defer_scaling_exchange = true;
				fi::twin_assemble_lumped(c);
				fi::chain_mark("finest: lumped replica");
			} catch (const fi::Fail& f) {
				main_code = f.code;
			} catch (...) {
				main_code = FI_ERR_HIP;
				fi::set_error("unexpected exception while building the lumped replica");
			}
		}
		if (helper) {
			helper->wait();
			fi::worker_pool().release(helper);
		} else if (main_code == FI_OK && !lumped) {
			build();
		}
		if (mixed64) {
			if (helper2) {
				helper2->wait();
				fi::worker_pool().release(helper2);
			} else if (main_code == FI_OK) {
				build2();
			}
			if (helper_code == FI_OK && helper2_code != FI_OK) {
				helper_code = helper2_code;
				helper_msg  = helper2_msg;
			}
		}
		fi::chain_mark("helpers joined");
		fi_ctx* const first_built = mixed64 ? c->twin : c->coarse;  // the replica, then its levels / the levels
		for (fi_ctx* l = first_built; l; l = l->coarse) { l->stream = c->stream; }
		const bool mine_ok = main_code == FI_OK && helper_code == FI_OK;
		bool peers_ok = true;
		try {
			peers_ok = fi::all_ranks_ok(c, mine_ok);  // (every rank gets here: nothing above is collective)
		} catch (const fi::Fail&) {
			peers_ok = false;
		}
		if (!mine_ok || !peers_ok) {
			(void)hipStreamSynchronize(c->level_stream);  // nothing of the helpers' work stays in flight behind the error
			if (c->level_stream2) { (void)hipStreamSynchronize(c->level_stream2); }
			c->defer_scaling_exchange = false;
			if (main_code != FI_OK) { throw fi::Fail{main_code}; }
			if (helper_code != FI_OK) {
				fi::set_error("%s", helper_msg.c_str());
				throw fi::Fail{helper_code};
			}
			fi::set_error("fi_assemble: another rank failed while assembling its slab");
			throw fi::Fail{FI_ERR_COMM};
		}
		if (fi::tuning_switch("FI_ASM_CHAIN_TIMES")) {  // (diagnostic: where each chain of the assembly ends, from the start event)
			hipEvent_t a = nullptr, b = nullptr, d = nullptr;
			FI_HIP_TRY(hipEventCreate(&a));
			FI_HIP_TRY(hipEventCreate(&b));
			FI_HIP_TRY(hipEventCreate(&d));
			FI_HIP_TRY(hipEventRecord(a, c->stream));
			FI_HIP_TRY(hipEventRecord(b, c->level_stream));
			if (mixed64) { FI_HIP_TRY(hipEventRecord(d, c->level_stream2)); }
			FI_HIP_TRY(hipEventSynchronize(a));
			FI_HIP_TRY(hipEventSynchronize(b));
			if (mixed64) { FI_HIP_TRY(hipEventSynchronize(d)); }
			float ta = 0, tb = 0, td = 0;
			(void)hipEventElapsedTime(&ta, e0, a);
			(void)hipEventElapsedTime(&tb, e0, b);
			if (mixed64) { (void)hipEventElapsedTime(&td, e0, d); }
			std::fprintf(stderr, "fi_assemble chains: solver stream %.3f ms, level stream %.3f ms, second level stream %.3f ms\n", ta, tb, td);
			(void)hipEventDestroy(a);
			(void)hipEventDestroy(b);
			(void)hipEventDestroy(d);
		}
		FI_HIP_TRY(hipEventRecord(c->ev_level, c->level_stream));
		FI_HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_level, 0));
		if (mixed64) {
			FI_HIP_TRY(hipEventRecord(c->ev_level2, c->level_stream2));
			FI_HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_level2, 0));
			fi::twin_finish(c);
		}
		// slabs: the levels' share of the assembly's one exchange (the diagonal's ghost planes), in level order on every rank
		fi::operator_finish_ghosts(c);
		for (fi_ctx* l = first_built; l; l = l->coarse) { fi::operator_finish_ghosts(l); }
	} else {
	fi::AllocStream alloc_on(c->stream);
	fi::assemble(c);
	fi::generic_assemble(c);
	fi::stencil_prepare(c);
	fi::operator_prepare(c);
	}
	if (beside) {
		if (!mixed64) { fi::build_twin(c); }  // (drops a replica left by an earlier, mixed assemble)
	} else if (mixed64) {  // the fp32 replica carries the levels
		const int keep = c->levels_wanted;
		c->levels_wanted = 0;
		fi::build_levels(c);
		c->levels_wanted = keep;
		fi::build_twin(c);
	} else {
		fi::build_levels(c);
		fi::build_twin(c);
	}
	FI_HIP_TRY(hipEventRecord(e1, c->stream));
	fi::chain_mark("fi_assemble returns");
	c->asm_time_pending   = true;
	c->stats.assemble_ms  = 0.0;
	c->stats.num_levels   = 1;
	for (fi_ctx* l = c->coarse; l; l = l->coarse) { c->stats.num_levels += 1; }
	if (c->twin) { c->stats.num_levels = c->twin->stats.num_levels; }
	c->stats.num_unknowns = c->g.nown;
	c->stats.spmv_bytes   = fi::apply_algorithmic_bytes(c);
	c->assembled          = true;
	c->vectors_ready      = false;
	FI_API_END
}

int fi_solve_cg(fi_ctx* c, const float* guess, int max_iterations, float tol, float* out, int* iterations,
                float* rel_residual, int memory)
{
	FI_API_BEGIN
	fi::check_assembled(c);
	fi::bind_device(c);
	fi::check_memory(memory);
	fi::AllocStream alloc_on(c->stream);  // (every level of a hierarchy solves on the finest level's stream)
	if (c->dtype == FI_F64) {
		fi::solve_cg_t<double>(c, guess, max_iterations, tol, out, iterations, rel_residual, memory);
	} else {
		fi::solve_cg_t<float>(c, guess, max_iterations, tol, out, iterations, rel_residual, memory);
	}
	FI_API_END
}

int fi_set_option(fi_ctx* c, int option, double value)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	switch (option) {
	case FI_OPT_VERIFY_RESIDUAL: c->verify_residual = value != 0.0; break;
	case FI_OPT_LEVELS:
		c->levels_wanted = value > 0 ? static_cast<int>(value) : 0;
		c->assembled = false;
		break;
	case FI_OPT_COARSE_TOLERANCE: c->coarse_tol = value > 0 ? value : 1e-3; break;
	case FI_OPT_MULTIGRID: c->mg_mode = value != 0.0 ? 1 : 0; break;
	case FI_OPT_MIXED_PRECISION:
		FI_REQUIRE(value == 0.0 || c->dtype == FI_F64, FI_ERR_INVALID, "FI_OPT_MIXED_PRECISION needs an FI_F64 context");
		c->mixed = value != 0.0 ? 1 : 0;
		c->assembled = false;
		break;
	case FI_OPT_POLY_TERMS:
		FI_REQUIRE(value >= 0 && value <= 32, FI_ERR_INVALID, "FI_OPT_POLY_TERMS must be 0..32");
		c->poly_terms = static_cast<int>(value);
		break;
	case FI_OPT_POLY_RATIO:
		FI_REQUIRE(value > 1.0 && value <= 1000.0, FI_ERR_INVALID, "FI_OPT_POLY_RATIO must be in (1, 1000]");
		c->poly_ratio = value;
		break;
	case FI_OPT_MG_SMOOTHER:
		c->mg_smoother = value != 0.0 ? 1 : 0;
		c->assembled = false;  // the levels take the setting when they are built
		break;
	case FI_OPT_MG_SAFE_FACTOR:
		FI_REQUIRE(value >= 1.0 && value <= 64.0, FI_ERR_INVALID, "FI_OPT_MG_SAFE_FACTOR must be 1..64");
		c->mg_safe = value;
		c->assembled = false;
		break;
	case FI_OPT_MG_TERMS:
		FI_REQUIRE(value >= 2 && value <= 16, FI_ERR_INVALID, "FI_OPT_MG_TERMS must be 2..16");
		c->mg_terms = static_cast<int>(value);
		c->assembled = false;  // the levels take the setting when they are built
		break;
	case FI_OPT_MG_RATIO:
		FI_REQUIRE(value > 1.0 && value <= 1000.0, FI_ERR_INVALID, "FI_OPT_MG_RATIO must be in (1, 1000]");
		c->mg_pratio = value;
		c->assembled = false;
		break;
	case FI_OPT_MG_CHEB_DEGREE:
		FI_REQUIRE(value == 0 || (value >= 2 && value <= 16), FI_ERR_INVALID, "FI_OPT_MG_CHEB_DEGREE must be 0 or 2..16");
		c->mg_cheb_degree = static_cast<int>(value);
		c->assembled = false;
		break;
	case FI_OPT_MG_CHEB_RATIO:
		FI_REQUIRE(value == 0 || (value > 1.0 && value <= 1000.0), FI_ERR_INVALID, "FI_OPT_MG_CHEB_RATIO must be 0 or in (1, 1000]");
		c->mg_cheb_ratio = value;
		c->assembled = false;
		break;
	case FI_OPT_MG_KCYCLE:
		FI_REQUIRE(value >= 0 && value <= 16, FI_ERR_INVALID, "FI_OPT_MG_KCYCLE must be 0..16");
		c->mg_kcycle = static_cast<int>(value);
		c->assembled = false;  // the levels take the setting when they are built
		break;
	case FI_OPT_FIELD_TOLERANCE:
		FI_REQUIRE(value >= 0.0 && value < 1.0, FI_ERR_INVALID, "FI_OPT_FIELD_TOLERANCE must be in [0, 1)");
		c->field_tol = value;
		break;
	default: FI_REQUIRE(false, FI_ERR_INVALID, "unknown option %d", option);
	}
	FI_API_END
}

int fi_jacobi(fi_ctx* c, const float* guess, int num_iterations, float weight, float* out, int memory)
{
	FI_API_BEGIN
	fi::check_assembled(c);
	fi::bind_device(c);
	fi::check_memory(memory);
	if (num_iterations < 0) { num_iterations = 0; }  // sparse_linear.cpp:220: returns the guess
	if (c->dtype == FI_F64) {
		fi::jacobi_t<double>(c, guess, num_iterations, weight, out, memory);
	} else {
		fi::jacobi_t<float>(c, guess, num_iterations, weight, out, memory);
	}
	FI_API_END
}

int fi_error_map(fi_ctx* c, const float* solution, float* out, int memory)
{
	FI_API_BEGIN
	fi::check_assembled(c);
	fi::bind_device(c);
	fi::check_memory(memory);
	FI_REQUIRE(solution && out, FI_ERR_INVALID, "fi_error_map needs a solution and an output buffer");
	fi::ensure_vectors(c);
	fi::RankSet R{c};
	if (c->dtype == FI_F64) {
		fi::load_owned<double>(c, c->x, solution, memory);
		fi::halo_exchange(R, &fi_ctx::x);
		fi::error_map(c, c->x.p, c->q.p);
		fi::store_owned<double>(c, c->q, out, memory);
	} else {
		fi::load_owned<float>(c, c->x, solution, memory);
		fi::halo_exchange(R, &fi_ctx::x);
		fi::error_map(c, c->x.p, c->q.p);
		fi::store_owned<float>(c, c->q, out, memory);
	}
	FI_API_END
}

// ---- robust fits (fi_robust.hip) ---------------------------------------------------------------------
int fi_point_count(const fi_ctx* c, long* n)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	FI_REQUIRE(n != nullptr, FI_ERR_INVALID, "null output");
	*n = fi::robust_point_count(c);
	FI_API_END
}

int fi_point_residuals(fi_ctx* c, const float* field, float* residuals, int memory)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	fi::bind_device(c);
	fi::check_memory(memory);
	fi::robust_residuals(c, field, residuals, memory);
	FI_API_END
}

int fi_robust_reweight(fi_ctx* c, const float* field, const fi_robust_options* options, float* omega, float* scale, int memory)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	fi::bind_device(c);
	FI_REQUIRE(options != nullptr, FI_ERR_INVALID, "options is null");
	fi::check_memory(memory);
	const fi::RobustStep step = fi::robust_reweight(c, field, options->loss, options->tuning, options->scale, omega, memory);
	if (scale) { *scale = step.scale; }
	FI_API_END
}

int fi_reset_point_weights(fi_ctx* c)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	fi::bind_device(c);
	fi::robust_reset(c);
	FI_API_END
}

int fi_solve_robust(fi_ctx* c, const float* guess, const fi_robust_options* options, int max_iterations, float tol, float* out,
                    float* omega, fi_robust_stats* stats, int memory)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	fi::bind_device(c);
	FI_REQUIRE(options != nullptr, FI_ERR_INVALID, "options is null");
	fi::check_memory(memory);
	FI_REQUIRE(options->rounds >= 0, FI_ERR_INVALID, "rounds = %d", options->rounds);
	FI_REQUIRE(options->weight_tolerance >= 0.0f, FI_ERR_INVALID, "weight_tolerance must be >= 0");
	const long n = fi::robust_check(c);  // (every refusal before any work)
	fi_robust_stats rs{};
	if (stats) { *stats = rs; }
	auto ok = [](int code) {  // the entry has left its message with fi_last_error
		if (code != FI_OK) { throw fi::Fail{code}; }
	};
	if (!c->assembled) { ok(fi_assemble(c)); }
	int it = 0;
	ok(fi_solve_cg(c, guess, max_iterations, tol, out, &it, nullptr, memory));
	rs.iterations = it;
	struct Start {  // the rounds start from the previous solution in the context's precision, kept beside the solver's vectors
		fi_ctx* c;
		~Start() { c->guess_native = nullptr; }
	} start{c};
	const size_t es = fi::elem_size(c);
	bool weighted = false;
	for (int round = 0; round < options->rounds; ++round) {
		const auto t0 = std::chrono::steady_clock::now();
		c->robust.xkeep.alloc(es * c->g.nown);
		FI_HIP_TRY(hipMemcpyAsync(c->robust.xkeep.p, static_cast<const char*>(c->x.p) + es * c->g.own_first, es * c->g.nown,
		                          hipMemcpyDeviceToDevice, c->stream));
		const fi::RobustStep step = fi::robust_reweight(c, nullptr, options->loss, options->tuning, options->scale, nullptr, memory);
		rs.reweight_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		rs.scale             = step.scale;
		rs.max_weight_change = step.max_weight_change;
		rs.points_used       = step.points_used;
		rs.points_zeroed     = step.points_zeroed;
		if (step.scale == 0.0f) { break; }  // nothing changed: the field is the fit of the weights the context holds
		weighted = true;
		ok(fi_assemble(c));
		c->guess_native = c->robust.xkeep.p;
		const int code = fi_solve_cg(c, nullptr, max_iterations, tol, out, &it, nullptr, memory);
		c->guess_native = nullptr;
		ok(code);
		rs.iterations += it;
		rs.rounds = round + 1;
		if (options->weight_tolerance > 0.0f && step.max_weight_change < options->weight_tolerance) { break; }
	}
	if (omega) {
		if (weighted || c->robust.n == n) {
			FI_HIP_TRY(hipMemcpy(omega, c->robust.omega.p, sizeof(float) * n, memory == FI_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
		} else {  // no step taken: every factor is 1
			std::vector<float> ones(static_cast<size_t>(n), 1.0f);
			FI_HIP_TRY(hipMemcpy(omega, ones.data(), sizeof(float) * n, memory == FI_HOST ? hipMemcpyHostToHost : hipMemcpyHostToDevice));
		}
	}
	if (stats) { *stats = rs; }
	FI_API_END
}

int fi_tile_pass(fi_ctx* c, const float* guess, int tile_size, float* out, int memory)
{
	FI_API_BEGIN
	fi::check_assembled(c);
	fi::bind_device(c);
	fi::check_memory(memory);
	FI_REQUIRE(tile_size >= 2, FI_ERR_INVALID, "tile_size %d < 2 (sparse_linear.cpp:254)", tile_size);
	FI_REQUIRE(guess && out, FI_ERR_INVALID, "fi_tile_pass needs a guess and an output buffer");
	FI_REQUIRE(c->nranks == 1 || c->generic.ntrip == 0, FI_ERR_UNSUPPORTED, "the tile pre-solver over triplet rows needs an undivided lattice");
	if (c->dtype == FI_F64) {
		fi::tile_pass_t<double>(c, guess, tile_size, out, memory);
	} else {
		fi::tile_pass_t<float>(c, guess, tile_size, out, memory);
	}
	FI_API_END
}

int fi_get_solution_f64(fi_ctx* c, double* out)
{
	FI_API_BEGIN
	fi::check_assembled(c);
	fi::bind_device(c);
	FI_REQUIRE(c->vectors_ready && out, FI_ERR_STATE, "no solution yet");
	c->dtype == FI_F64 ? fi::get_vec_f64_t<double>(c, c->x, out) : fi::get_vec_f64_t<float>(c, c->x, out);
	FI_API_END
}

int fi_true_residual(fi_ctx* c, double* rel)
{
	FI_API_BEGIN
	fi::check_assembled(c);
	fi::bind_device(c);
	FI_REQUIRE(rel != nullptr, FI_ERR_INVALID, "null output");
	*rel = c->dtype == FI_F64 ? fi::true_residual_t<double>(c) : fi::true_residual_t<float>(c);
	FI_API_END
}

int fi_apply_AtA_f64(fi_ctx* c, const double* x, double* y)
{
	FI_API_BEGIN
	fi::check_assembled(c);
	fi::bind_device(c);
	FI_REQUIRE(x && y, FI_ERR_INVALID, "null vector");
	c->dtype == FI_F64 ? fi::apply_f64_t<double>(c, x, y) : fi::apply_f64_t<float>(c, x, y);
	FI_API_END
}

int fi_get_Atb_f64(fi_ctx* c, double* out)
{
	FI_API_BEGIN
	fi::check_assembled(c);
	fi::bind_device(c);
	c->dtype == FI_F64 ? fi::get_vec_f64_t<double>(c, c->atb, out) : fi::get_vec_f64_t<float>(c, c->atb, out);
	FI_API_END
}

int fi_get_diag_f64(fi_ctx* c, double* out)
{
	FI_API_BEGIN
	fi::check_assembled(c);
	fi::bind_device(c);
	c->dtype == FI_F64 ? fi::get_vec_f64_t<double>(c, c->diag, out) : fi::get_vec_f64_t<float>(c, c->diag, out);
	FI_API_END
}

int fi_get_stats(const fi_ctx* c, fi_stats* out)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "null output");
	fi::finish_assemble_timing(const_cast<fi_ctx*>(c));
	*out = c->stats;
	// Levels of the coarse-to-fine start that were solved without a look at their stop flag (cg_run, `unwatched`) reported
	// the PREDICTED iteration count; the flag's copy has reached pinned memory since (the finest level's solve ended with a
	// synchronisation behind it): the caller gets what the levels really did, and `coarse_unconverged` says how many of
	// them had not met their tolerance after the predicted steps (their start guess was that much poorer, nothing else).
	out->coarse_unconverged = 0;
	const fi_ctx* top = c->twin && c->twin->coarse ? c->twin : c;
	for (const fi_ctx* l = top->coarse; l; l = l->coarse) {
		if (!l->unwatched_pending || !l->ev_unwatched || !l->pin[2]) { continue; }
		if (hipEventSynchronize(l->ev_unwatched) != hipSuccess) { continue; }
		const fi::CgScalars* was = static_cast<const fi::CgScalars*>(l->pin[2]);
		const bool met = was->done == 1 || was->done == 5 || was->done == 4;
		if (!met) { out->coarse_unconverged += 1; }
		out->coarse_iterations += (met ? was->iter : l->unwatched_expected) - l->unwatched_expected;
	}
	FI_API_END
}

int fi_time_apply(fi_ctx* c, int reps, double* ms_per_launch)
{
	FI_API_BEGIN
	fi::check_assembled(c);
	fi::bind_device(c);
	FI_REQUIRE(reps > 0 && ms_per_launch, FI_ERR_INVALID, "bad arguments");
	fi::ensure_vectors(c);
	fi::CgScalars init{};
	FI_HIP_TRY(hipMemcpyAsync(c->scal.p, &init, sizeof(init), hipMemcpyHostToDevice, c->stream));
	fi::EventPair timer;  // (destroyed on every way out: a coarse level's breakdown, a timeout)
	const hipEvent_t e0 = timer.e0, e1 = timer.e1;
	// timing builds: FI_TIME_STEP = 1 / 2 / 3 times that step of the polynomial preconditioner instead (operands: the
	// solver's vectors as they are -- isolated launches, the numbers of profiles/r2_ablation.md)
	const char* which = fi::tuning_switch("FI_TIME_STEP");
	const int   step = which ? atoi(which) : 0;
	auto launch = [&]() {
		if (step >= 1 && fi::stencil_cheb_available(c)) {
			c->dtype == FI_F64 ? fi::ensure_poly_vectors<double>(c) : fi::ensure_poly_vectors<float>(c);
			if (step == 1) {
				fi::stencil_cheb_step(c, c->r.p, nullptr, c->r.p, c->mg_d.p, 0.3, 0.2, c->partial.as<double>(), 0, 0.0, 0.5);
			} else if (step == 2) {
				fi::stencil_cheb_step(c, c->mg_d.p, c->mg_x.p, c->r.p, c->mg_x.p, 0.3, 0.2, c->partial.as<double>(), 0, 0.5);
			} else {
				fi::stencil_cheb_step(c, c->mg_x.p, c->mg_d.p, c->r.p, c->mg_d.p, 0.3, 0.2, c->partial.as<double>());
			}
		} else {
			fi::apply_AtA(c, c->p.p, c->q.p, c->partial.as<double>());
		}
	};
	launch();  // warm-up
	FI_HIP_TRY(hipEventRecord(e0, c->stream));
	for (int k = 0; k < reps; ++k) { launch(); }
	FI_HIP_TRY(hipEventRecord(e1, c->stream));
	FI_HIP_TRY(hipEventSynchronize(e1));
	float ms = 0;
	FI_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
	*ms_per_launch = ms / reps;
	FI_API_END
}

int fi_upscale_field(const float* small_field, int ndim, const int* small_sizes, const int* large_sizes, float* out,
                     int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(small_field && small_sizes && large_sizes && out, FI_ERR_INVALID, "null argument");
	FI_REQUIRE(1 <= ndim && ndim <= FI_MAX_DIM, FI_ERR_INVALID, "ndim must be 1..3");
	fi::check_memory(memory);
	fi::UpscaleArgs a{};
	a.ndim = ndim;
	int64_t ns = 1, nl = 1;
	for (int d = 0; d < ndim; ++d) {
		FI_REQUIRE(small_sizes[d] >= 1 && large_sizes[d] >= 1, FI_ERR_INVALID, "bad size");
		a.ssz[d] = small_sizes[d];
		a.lsz[d] = large_sizes[d];
		ns *= small_sizes[d];
		nl *= large_sizes[d];
	}
	fi::stage::In<float>  s(small_field, ns, memory, nullptr);
	fi::stage::Out<float> o(out, nl, memory);
	hipLaunchKernelGGL(fi::k_upscale, dim3(fi::blocks_for(nl)), dim3(fi::kThreads), 0, nullptr, a, nl, s.dev, o.dev);
	FI_HIP_TRY(hipGetLastError());
	o.back(nullptr);
	FI_HIP_TRY(hipDeviceSynchronize());
	FI_API_END
}


// ---- iso-contours (fi_iso.hip) ------------------------------------------------------------------
int fi_iso_extract(fi_ctx* c, const float* field, float iso, int memory, fi_mesh** out)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "out is null");
	*out = nullptr;
	fi::bind_device(c);
	fi::iso_extract_ctx(c, field, iso, memory, out);
	FI_API_END
}

int fi_iso_extract_field(const float* field, int ndim, const int* sizes, float iso, int memory, fi_mesh** out)
{
	FI_API_BEGIN
	FI_REQUIRE(field && sizes && out, FI_ERR_INVALID, "null argument");
	fi::check_memory(memory);
	*out = nullptr;
	FI_REQUIRE(ndim != 1, FI_ERR_UNSUPPORTED, "iso-contours of a 1-D lattice are not supported");
	FI_REQUIRE(ndim == 2 || ndim == 3, FI_ERR_INVALID, "ndim must be 2 or 3 (got %d)", ndim);
	const int64_t n = fi::lattice_points(ndim, sizes);
	fi::stage::In<float> f(field, n, memory, nullptr);
	fi::iso_extract_whole(f, ndim, sizes, iso, 1, nullptr, nullptr, nullptr, out);
	FI_API_END
}

// ---- dual contouring (fi_dual.hip) --------------------------------------------------------------
int fi_dual_contour(fi_ctx* c, const float* field, const float* gradients, float iso, int memory, fi_mesh** out)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "out is null");
	*out = nullptr;
	fi::bind_device(c);
	fi::dual_contour_ctx(c, field, gradients, iso, memory, out);
	FI_API_END
}

int fi_dual_contour_field(const float* field, const float* gradients, int ndim, const int* sizes, float iso, int memory,
                          fi_mesh** out)
{
	FI_API_BEGIN
	FI_REQUIRE(field && sizes && out, FI_ERR_INVALID, "null argument");
	fi::check_memory(memory);
	*out = nullptr;
	FI_REQUIRE(ndim != 1, FI_ERR_UNSUPPORTED, "dual contouring of a 1-D lattice is not supported");
	FI_REQUIRE(ndim == 2 || ndim == 3, FI_ERR_INVALID, "ndim must be 2 or 3 (got %d)", ndim);
	const int64_t n = fi::lattice_points(ndim, sizes);
	fi::stage::In<float> f(field, n, memory, nullptr), g(gradients, ndim * n, memory, nullptr);
	fi::dual_contour_whole(f, g, ndim, sizes, iso, nullptr, out);
	FI_API_END
}

int fi_mesh_info(const fi_mesh* m, long* num_vertices, long* num_primitives, int* vertices_per_primitive)
{
	FI_API_BEGIN
	FI_REQUIRE(m != nullptr, FI_ERR_INVALID, "null mesh");
	if (num_vertices) { *num_vertices = static_cast<long>(m->nv); }
	if (num_primitives) { *num_primitives = static_cast<long>(m->np); }
	if (vertices_per_primitive) { *vertices_per_primitive = m->ndim; }
	FI_API_END
}

int fi_mesh_copy(const fi_mesh* m, float* vertices, float* normals, int* indices, long long* keys, int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(m != nullptr, FI_ERR_INVALID, "null mesh");
	fi::check_memory(memory);
	FI_HIP_TRY(hipSetDevice(m->device));
	const hipMemcpyKind kind = memory == FI_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
	const size_t nv = static_cast<size_t>(m->nv), np = static_cast<size_t>(m->np), D = static_cast<size_t>(m->ndim);
	if (vertices && nv) { FI_HIP_TRY(hipMemcpy(vertices, m->pos.p, sizeof(float) * D * nv, kind)); }
	FI_REQUIRE(!normals || m->has_normals, FI_ERR_INVALID, "the mesh has no normals");
	if (normals && nv) { FI_HIP_TRY(hipMemcpy(normals, m->nrm.p, sizeof(float) * D * nv, kind)); }
	if (indices && np) { FI_HIP_TRY(hipMemcpy(indices, m->idx.p, sizeof(int) * D * np, kind)); }
	if (keys && nv) { FI_HIP_TRY(hipMemcpy(keys, m->key.p, sizeof(int64_t) * nv, kind)); }
	FI_API_END
}

int fi_mesh_destroy(fi_mesh* m) { return fi::destroy_handle(m); }

// ---- the connected parts of a mesh (fi_parts.hip) -------------------------------------------------
int fi_mesh_create(fi_mesh** out, int ndim, long num_vertices, const float* vertices, const float* normals, const long long* keys,
                   long num_primitives, const int* indices, int memory)
{
	FI_API_BEGIN
	fi::mesh_create(out, ndim, num_vertices, vertices, normals, keys, num_primitives, indices, memory);
	FI_API_END
}

int fi_mesh_parts(const fi_mesh* m, long* num_parts, int* vertex_labels, int* primitive_labels, int memory)
{
	FI_API_BEGIN
	fi::mesh_parts(m, num_parts, vertex_labels, primitive_labels, memory);
	FI_API_END
}

int fi_mesh_measure(const fi_mesh* m, long capacity, fi_mesh_part* parts, long* num_parts)
{
	FI_API_BEGIN
	fi::mesh_measure(m, capacity, parts, num_parts);
	FI_API_END
}

int fi_mesh_select(const fi_mesh* m, long num_parts, const unsigned char* keep, fi_mesh** out)
{
	FI_API_BEGIN
	fi::mesh_select(m, num_parts, keep, out);
	FI_API_END
}

// ---- mesh simplification (fi_simplify.hip) ----------------------------------------------------------
int fi_mesh_simplify(const fi_mesh* m, float cell, const float* origin, int placement, int* vertex_map, int memory, fi_mesh** out)
{
	FI_API_BEGIN
	fi::mesh_simplify(m, cell, origin, placement, vertex_map, memory, out);
	FI_API_END
}

// ---- mesh smoothing (fi_smooth.hip) -------------------------------------------------------------------
int fi_mesh_smooth(const fi_mesh* m, const fi_smooth_options* opt, fi_mesh** out)
{
	FI_API_BEGIN
	fi::mesh_smooth(m, opt, out);
	FI_API_END
}

int fi_mesh_normals(const fi_mesh* m, fi_mesh** out)
{
	FI_API_BEGIN
	fi::mesh_normals(m, out);
	FI_API_END
}

// ---- points on a mesh, mesh-to-surface deviation (fi_meshpts.hip) ---------------------------------------
int fi_mesh_sample(const fi_mesh* m, long n, unsigned long long seed, int normals_mode, float* positions, float* normals,
                   long long* primitives, int memory)
{
	FI_API_BEGIN
	fi::mesh_sample(m, n, seed, normals_mode, positions, normals, primitives, memory);
	FI_API_END
}

int fi_mesh_deviation(const fi_mesh* a, fi_surface* b, long samples, unsigned long long seed, float max_distance, fi_deviation* of_samples,
                      fi_deviation* of_vertices, float* vertex_distances, int memory)
{
	FI_API_BEGIN
	fi::mesh_deviation(a, b, samples, seed, max_distance, of_samples, of_vertices, vertex_distances, memory);
	FI_API_END
}

// ---- rigid registration of a point cloud (fi_register.hip) ---------------------------------------------
int fi_mesh_register(const fi_mesh* target, fi_surface* index, long n, const float* source, const fi_register_options* options,
                     const double* initial, fi_registration* out, float* transformed, float* distances, int memory)
{
	FI_API_BEGIN
	fi::mesh_register(target, index, n, source, options, initial, out, transformed, distances, memory);
	FI_API_END
}

int fi_points_register(const fi_points* target, const float* target_normals, long n, const float* source,
                       const fi_register_options* options, const double* initial, fi_registration* out, float* transformed,
                       float* distances, int memory)
{
	FI_API_BEGIN
	fi::points_register(target, target_normals, n, source, options, initial, out, transformed, distances, memory);
	FI_API_END
}

// ---- point queries (fi_sample.hip) --------------------------------------------------------------
int fi_sample(fi_ctx* c, const float* field, long n, const float* positions, int mode, float fill, float* values,
              float* gradients, int memory)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	fi::bind_device(c);
	fi::sample_ctx(c, field, static_cast<int64_t>(n), positions, mode, fill, values, gradients, memory);
	FI_API_END
}

int fi_sample_field(const float* field, int ndim, const int* sizes, long n, const float* positions, int mode, float fill,
                    float* values, float* gradients, int memory)
{
	FI_API_BEGIN
	fi::sample_field(field, ndim, sizes, static_cast<int64_t>(n), positions, mode, fill, values, gradients, memory);
	FI_API_END
}


// ---- nearest data points (fi_nearest.hip) -------------------------------------------------------
namespace {
void check_nearest(long n, const float* queries, float max_distance, const float* distances, int memory)
{
	FI_REQUIRE(n >= 0, FI_ERR_INVALID, "n = %ld", n);
	FI_REQUIRE(queries != nullptr && distances != nullptr, FI_ERR_INVALID, "null queries or distances");
	FI_REQUIRE(max_distance >= 0.0f, FI_ERR_INVALID, "max_distance must be >= 0 (got %g)", static_cast<double>(max_distance));  // (NaN fails)
	fi::check_memory(memory);
	// (one thread per query, 32-bit counts)
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld queries in one call", n);
}

void check_field_out(float max_distance, const float* out, int memory)
{
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "out is null");
	FI_REQUIRE(max_distance >= 0.0f, FI_ERR_INVALID, "max_distance must be >= 0 (got %g)", static_cast<double>(max_distance));
	fi::check_memory(memory);
}

void check_points(const fi_points* h)
{
	FI_REQUIRE(h != nullptr, FI_ERR_INVALID, "point set is null");
	FI_HIP_TRY(hipSetDevice(h->device));
}

// The point set of a call: the data points of a context (fi_<op>) or a set of its own (fi_points_<op>).  Every operation
// on a point set is written once below, over this; its two exported names only say which handle they were given.  A body
// goes: bind(), the operation's own argument checks, whole(), index().
struct PointSet {
	fi_ctx*          c = nullptr;
	const fi_points* h = nullptr;
	const bool       of_ctx;
	PointSet(fi_ctx* c_) : c(c_), of_ctx(true) {}
	PointSet(const fi_points* h_) : h(h_), of_ctx(false) {}

	// a null handle refused; the handle's device current
	void bind() const
	{
		if (!of_ctx) { return check_points(h); }
		fi::check_ctx(c);
		fi::bind_device(c);
	}
	int         ndim() const { return of_ctx ? c->g.ndim : h->t.D; }
	hipStream_t stream() const { return of_ctx ? c->stream : nullptr; }
	// the border prior's reason: a slab context holds only the points near its slab
	void whole() const
	{
		FI_REQUIRE(!of_ctx || c->nranks == 1, FI_ERR_UNSUPPORTED, "nearest points on a slab context: a rank sees only its own points");
	}
	// (a context's is built here, at the first call that comes this far)
	const fi::NearestIndex& index() const { return of_ctx ? fi::nearest_of(c) : h->t; }
};

int points_nearest(PointSet s, long n, const float* queries, float max_distance, float* distances, long long* indices, int memory)
{
	FI_API_BEGIN
	s.bind();
	check_nearest(n, queries, max_distance, distances, memory);
	s.whole();
	// before a context builds its index; nothing changes for a set of its own: nearest_query's first line is this return
	if (n == 0) { return FI_OK; }
	fi::nearest_query(s.index(), n, queries, max_distance, distances, indices, memory, s.stream());
	FI_API_END
}

// sizes: the lattice of a set of its own; a context brings its lattice
int points_distance_field(PointSet s, const int* sizes, float max_distance, float* out, long long* indices, int memory)
{
	FI_API_BEGIN
	s.bind();
	if (s.of_ctx) {
		sizes = s.c->g.gn;
	} else {
		FI_REQUIRE(sizes != nullptr, FI_ERR_INVALID, "sizes is null");
		for (int d = 0; d < s.ndim(); ++d) { FI_REQUIRE(sizes[d] >= 1, FI_ERR_INVALID, "sizes[%d] = %d", d, sizes[d]); }
	}
	check_field_out(max_distance, out, memory);
	s.whole();
	fi::nearest_lattice(s.index(), sizes, max_distance, out, indices, memory, s.stream());
	FI_API_END
}
}  // namespace

int fi_nearest(fi_ctx* c, long n, const float* queries, float max_distance, float* distances, long long* indices, int memory)
{
	return points_nearest(c, n, queries, max_distance, distances, indices, memory);
}

int fi_points_nearest(fi_points* h, long n, const float* queries, float max_distance, float* distances, long long* indices,
                      int memory)
{
	return points_nearest(h, n, queries, max_distance, distances, indices, memory);
}

int fi_distance_field(fi_ctx* c, float max_distance, float* out, long long* indices, int memory)
{
	return points_distance_field(c, nullptr, max_distance, out, indices, memory);
}

int fi_points_distance_field(fi_points* h, const int* sizes, float max_distance, float* out, long long* indices, int memory)
{
	return points_distance_field(h, sizes, max_distance, out, indices, memory);
}

int fi_points_create(fi_points** out, int ndim, long n, const float* positions, int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "out is null");
	*out = nullptr;
	FI_REQUIRE(1 <= ndim && ndim <= FI_MAX_DIM, FI_ERR_INVALID, "ndim must be 1..%d (got %d)", FI_MAX_DIM, ndim);
	FI_REQUIRE(n >= 0, FI_ERR_INVALID, "n = %ld", n);
	FI_REQUIRE(n == 0 || positions != nullptr, FI_ERR_INVALID, "positions is null");
	fi::check_memory(memory);
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld points: nearest-point indices are 32-bit", n);
	std::unique_ptr<fi_points> h(new fi_points());
	FI_HIP_TRY(hipGetDevice(&h->device));
	fi::stage::In<float> pos(n > 0 ? positions : nullptr, static_cast<int64_t>(ndim) * n, memory, nullptr);
	const float*  p   = pos;
	const int64_t cnt = n;
	fi::nearest_build(h->t, ndim, cnt, &p, &cnt, 1, nullptr);
	*out = h.release();
	FI_API_END
}

int fi_points_destroy(fi_points* h) { return fi::destroy_handle(h); }


// ---- k nearest data points; normals from them (fi_knn.hip) --------------------------------------
namespace {
void check_k(int k)
{
	FI_REQUIRE(1 <= k && k <= fi::kMaxNeighbours, FI_ERR_INVALID, "k must be 1..%d (got %d)", fi::kMaxNeighbours, k);
}

// The arguments of fi_estimate_normals and fi_orient_normals that need no point set.  `mode` is the argument that says what the
// guides are, under the name the operation's sentences give it; `fit`: a plane is fitted to the k neighbours.
void check_normals(const char* mode_name, bool fit, int ndim, int k, float max_distance, int mode, const float* normals, int memory)
{
	FI_REQUIRE(ndim >= 2, FI_ERR_INVALID, "normals need 2 or 3 dimensions (got %d)", ndim);
	check_k(k);
	FI_REQUIRE(!fit || k >= ndim, FI_ERR_INVALID, "k = %d neighbours span no plane in %d dimensions", k, ndim);
	FI_REQUIRE(normals != nullptr, FI_ERR_INVALID, "normals is null");
	FI_REQUIRE(max_distance >= 0.0f, FI_ERR_INVALID, "max_distance must be >= 0 (got %g)", static_cast<double>(max_distance));
	fi::check_memory(memory);
	FI_REQUIRE(mode == FI_ORIENT_NONE || mode == FI_ORIENT_VIEWPOINTS || mode == FI_ORIENT_DIRECTIONS, FI_ERR_INVALID, "bad %s %d",
	           mode_name, mode);
}

// ... and the guides against the set's size, once its index is there
void check_guides(const char* mode_name, const fi::NearestIndex& t, int mode, const float* guides, long num_guides)
{
	if (mode == FI_ORIENT_NONE) { return; }
	FI_REQUIRE(guides != nullptr, FI_ERR_INVALID, "%s %d without guides", mode_name, mode);
	FI_REQUIRE(num_guides == t.n || (mode == FI_ORIENT_VIEWPOINTS && num_guides == 1), FI_ERR_INVALID, "%ld guides for %lld points",
	           num_guides, static_cast<long long>(t.n));
}

int points_knn(PointSet s, long n, const float* queries, int k, float max_distance, float* distances, long long* indices, int memory)
{
	FI_API_BEGIN
	s.bind();
	check_nearest(n, queries, max_distance, distances, memory);
	check_k(k);
	s.whole();
	if (n == 0) { return FI_OK; }  // (as in points_nearest: knn_query's first line)
	fi::knn_query(s.index(), n, queries, k, max_distance, distances, indices, memory, s.stream());
	FI_API_END
}

int points_estimate_normals(PointSet s, int k, float max_distance, int orient, const float* guides, long num_guides, float* normals,
                            float* variation, int memory)
{
	FI_API_BEGIN
	s.bind();
	check_normals("orientation mode", true, s.ndim(), k, max_distance, orient, normals, memory);
	s.whole();
	const fi::NearestIndex& t = s.index();
	check_guides("orientation mode", t, orient, guides, num_guides);
	fi::estimate_normals(t, k, max_distance, orient, guides, num_guides, normals, variation, memory, s.stream());
	FI_API_END
}
}  // namespace

int fi_knn(fi_ctx* c, long n, const float* queries, int k, float max_distance, float* distances, long long* indices, int memory)
{
	return points_knn(c, n, queries, k, max_distance, distances, indices, memory);
}

int fi_points_knn(fi_points* h, long n, const float* queries, int k, float max_distance, float* distances, long long* indices,
                  int memory)
{
	return points_knn(h, n, queries, k, max_distance, distances, indices, memory);
}

int fi_estimate_normals(fi_ctx* c, int k, float max_distance, int orient, const float* guides, long num_guides, float* normals,
                        float* variation, int memory)
{
	return points_estimate_normals(c, k, max_distance, orient, guides, num_guides, normals, variation, memory);
}

int fi_points_estimate_normals(fi_points* h, int k, float max_distance, int orient, const float* guides, long num_guides,
                               float* normals, float* variation, int memory)
{
	return points_estimate_normals(h, k, max_distance, orient, guides, num_guides, normals, variation, memory);
}


// ---- a point cloud made smooth: moving-least-squares projection (fi_mls.hip) ----------------------
namespace {
void check_mls(int ndim, long n, const float* queries, int k, float radius, int degree, float max_move, bool any_output, int memory)
{
	FI_REQUIRE(ndim >= 2, FI_ERR_INVALID, "a local surface needs 2 or 3 dimensions (got %d)", ndim);
	check_k(k);
	// (every comparison is false for a NaN)
	FI_REQUIRE(radius > 0.0f && std::isfinite(radius), FI_ERR_INVALID, "radius must be > 0 and finite (got %g)", static_cast<double>(radius));
	FI_REQUIRE(degree == 1 || degree == 2, FI_ERR_INVALID, "degree must be 1 or 2 (got %d)", degree);
	FI_REQUIRE(max_move >= 0.0f, FI_ERR_INVALID, "max_move must be >= 0 (got %g)", static_cast<double>(max_move));
	fi::check_memory(memory);
	FI_REQUIRE(any_output, FI_ERR_INVALID, "every output is null");
	if (!queries) { return; }
	FI_REQUIRE(n >= 0, FI_ERR_INVALID, "n = %ld", n);
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld queries in one call", n);  // (one thread per query)
}

int points_mls_project(PointSet s, long n, const float* queries, int k, float radius, int degree, float max_move, const float* guide_normals,
                       float* positions, float* normals, float* curvature, unsigned char* order, int memory)
{
	FI_API_BEGIN
	s.bind();
	check_mls(s.ndim(), n, queries, k, radius, degree, max_move, positions || normals || curvature || order, memory);
	s.whole();
	fi::mls_project(s.index(), n, queries, k, radius, degree, max_move, guide_normals, positions, normals, curvature, order, memory, s.stream());
	FI_API_END
}
}  // namespace

int fi_mls_project(fi_ctx* c, long n, const float* queries, int k, float radius, int degree, float max_move, const float* guide_normals,
                   float* positions, float* normals, float* curvature, unsigned char* order, int memory)
{
	return points_mls_project(c, n, queries, k, radius, degree, max_move, guide_normals, positions, normals, curvature, order, memory);
}

int fi_points_mls_project(fi_points* h, long n, const float* queries, int k, float radius, int degree, float max_move,
                          const float* guide_normals, float* positions, float* normals, float* curvature, unsigned char* order, int memory)
{
	return points_mls_project(h, n, queries, k, radius, degree, max_move, guide_normals, positions, normals, curvature, order, memory);
}


// ---- a point cloud made clean: thinning and outlier removal (fi_cloud.hip) -----------------------
namespace {
void check_radius(float radius, int least, const char* what, int memory)
{
	FI_REQUIRE(radius >= 0.0f, FI_ERR_INVALID, "radius must be >= 0 (got %g)", static_cast<double>(radius));  // (NaN fails)
	FI_REQUIRE(least >= 1, FI_ERR_INVALID, "%s must be >= 1 (got %d)", what, least);
	fi::check_memory(memory);
}

void check_radius_count(long n, const float* queries, float radius, int limit, const int* counts, int memory)
{
	FI_REQUIRE(n >= 0, FI_ERR_INVALID, "n = %ld", n);
	FI_REQUIRE(queries != nullptr && counts != nullptr, FI_ERR_INVALID, "null queries or counts");
	check_radius(radius, limit, "limit", memory);
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld queries in one call", n);  // (one thread per query, 32-bit counts)
}

void check_neighbours(int k, float max_distance, bool any_output, int memory)
{
	check_k(k);
	FI_REQUIRE(max_distance >= 0.0f, FI_ERR_INVALID, "max_distance must be >= 0 (got %g)", static_cast<double>(max_distance));
	fi::check_memory(memory);
	FI_REQUIRE(any_output, FI_ERR_INVALID, "every output is null");
}

void check_statistical(int k, float max_distance, float std_ratio, bool any_output, int memory)
{
	check_neighbours(k, max_distance, any_output, memory);
	FI_REQUIRE(std_ratio >= 0.0f, FI_ERR_INVALID, "std_ratio must be >= 0 (got %g)", static_cast<double>(std_ratio));
}

int points_radius_count(PointSet s, long n, const float* queries, float radius, int limit, int* counts, int memory)
{
	FI_API_BEGIN
	s.bind();
	check_radius_count(n, queries, radius, limit, counts, memory);
	s.whole();
	if (n == 0) { return FI_OK; }  // (as in points_nearest: cloud_radius_count's first line)
	fi::cloud_radius_count(s.index(), n, queries, radius, limit, counts, memory, s.stream());
	FI_API_END
}

int points_neighbour_distances(PointSet s, int k, float max_distance, float* mean, float* kth, int* counts, int memory)
{
	FI_API_BEGIN
	s.bind();
	check_neighbours(k, max_distance, mean || kth || counts, memory);
	s.whole();
	fi::cloud_neighbour_distances(s.index(), k, max_distance, mean, kth, counts, memory, s.stream());
	FI_API_END
}

int points_outliers_statistical(PointSet s, int k, float max_distance, float std_ratio, unsigned char* keep, fi_outlier_stats* stats,
                                int memory)
{
	FI_API_BEGIN
	s.bind();
	check_statistical(k, max_distance, std_ratio, keep || stats, memory);
	s.whole();
	fi::cloud_outliers_statistical(s.index(), k, max_distance, std_ratio, keep, stats, memory, s.stream());
	FI_API_END
}

int points_outliers_radius(PointSet s, float radius, int min_neighbours, unsigned char* keep, long* num_kept, int memory)
{
	FI_API_BEGIN
	s.bind();
	check_radius(radius, min_neighbours, "min_neighbours", memory);
	FI_REQUIRE(keep || num_kept, FI_ERR_INVALID, "every output is null");
	s.whole();
	fi::cloud_outliers_radius(s.index(), radius, min_neighbours, keep, num_kept, memory, s.stream());
	FI_API_END
}
}  // namespace

int fi_radius_count(fi_ctx* c, long n, const float* queries, float radius, int limit, int* counts, int memory)
{
	return points_radius_count(c, n, queries, radius, limit, counts, memory);
}

int fi_points_radius_count(fi_points* h, long n, const float* queries, float radius, int limit, int* counts, int memory)
{
	return points_radius_count(h, n, queries, radius, limit, counts, memory);
}

int fi_neighbour_distances(fi_ctx* c, int k, float max_distance, float* mean, float* kth, int* counts, int memory)
{
	return points_neighbour_distances(c, k, max_distance, mean, kth, counts, memory);
}

int fi_points_neighbour_distances(fi_points* h, int k, float max_distance, float* mean, float* kth, int* counts, int memory)
{
	return points_neighbour_distances(h, k, max_distance, mean, kth, counts, memory);
}

int fi_outliers_statistical(fi_ctx* c, int k, float max_distance, float std_ratio, unsigned char* keep, fi_outlier_stats* stats, int memory)
{
	return points_outliers_statistical(c, k, max_distance, std_ratio, keep, stats, memory);
}

int fi_points_outliers_statistical(fi_points* h, int k, float max_distance, float std_ratio, unsigned char* keep, fi_outlier_stats* stats,
                                   int memory)
{
	return points_outliers_statistical(h, k, max_distance, std_ratio, keep, stats, memory);
}

int fi_outliers_radius(fi_ctx* c, float radius, int min_neighbours, unsigned char* keep, long* num_kept, int memory)
{
	return points_outliers_radius(c, radius, min_neighbours, keep, num_kept, memory);
}

int fi_points_outliers_radius(fi_points* h, float radius, int min_neighbours, unsigned char* keep, long* num_kept, int memory)
{
	return points_outliers_radius(h, radius, min_neighbours, keep, num_kept, memory);
}

int fi_cloud_thin(int ndim, long n, const float* positions, const float* normals, const float* values, float cell, const float* origin,
                  int mode, float* out_positions, float* out_normals, float* out_values, int* out_counts, long long* out_indices,
                  int* cell_map, long* num_out, int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(num_out != nullptr, FI_ERR_INVALID, "num_out is null");
	*num_out = 0;
	FI_REQUIRE(1 <= ndim && ndim <= FI_MAX_DIM, FI_ERR_INVALID, "ndim must be 1..%d (got %d)", FI_MAX_DIM, ndim);
	FI_REQUIRE(n >= 0, FI_ERR_INVALID, "n = %ld", n);
	FI_REQUIRE(n == 0 || (positions != nullptr && out_positions != nullptr), FI_ERR_INVALID, "null positions or out_positions");
	FI_REQUIRE(normals != nullptr || out_normals == nullptr, FI_ERR_INVALID, "out_normals without normals");
	FI_REQUIRE(values != nullptr || out_values == nullptr, FI_ERR_INVALID, "out_values without values");
	FI_REQUIRE(cell > 0.0f, FI_ERR_INVALID, "cell must be > 0 (got %g)", static_cast<double>(cell));  // (false for a NaN)
	FI_REQUIRE(mode == FI_THIN_MEAN || mode == FI_THIN_FIRST, FI_ERR_INVALID, "bad mode %d", mode);
	fi::check_memory(memory);
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld points in one call", n);
	fi::cloud_thin(ndim, n, positions, normals, values, cell, origin, mode, out_positions, out_normals, out_values, out_counts, out_indices,
	               cell_map, num_out, memory);
	FI_API_END
}


// ---- the clusters of a point cloud (fi_cluster.hip) ----------------------------------------------
namespace {
void check_cluster(float eps, int min_points, const int* labels, const fi_cluster_stats* stats, int memory)
{
	FI_REQUIRE(eps >= 0.0f && !std::isinf(eps), FI_ERR_INVALID, "eps must be finite and >= 0 (got %g)", static_cast<double>(eps));  // (NaN fails)
	FI_REQUIRE(min_points >= 1, FI_ERR_INVALID, "min_points must be >= 1 (got %d)", min_points);
	fi::check_memory(memory);
	FI_REQUIRE(labels || stats, FI_ERR_INVALID, "every output is null");
}

int points_cluster(PointSet s, float eps, int min_points, int* labels, unsigned char* core, fi_cluster_stats* stats, int memory)
{
	FI_API_BEGIN
	s.bind();
	check_cluster(eps, min_points, labels, stats, memory);
	s.whole();
	fi::cluster_labels(s.index(), eps, min_points, labels, core, stats, memory, s.stream());
	FI_API_END
}
}  // namespace

int fi_cluster(fi_ctx* c, float eps, int min_points, int* labels, unsigned char* core, fi_cluster_stats* stats, int memory)
{
	return points_cluster(c, eps, min_points, labels, core, stats, memory);
}

int fi_points_cluster(fi_points* h, float eps, int min_points, int* labels, unsigned char* core, fi_cluster_stats* stats, int memory)
{
	return points_cluster(h, eps, min_points, labels, core, stats, memory);
}

int fi_cluster_measure(int ndim, long n, const float* positions, const int* labels, const unsigned char* core, long num_clusters,
                       fi_cluster_row* rows, int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(1 <= ndim && ndim <= FI_MAX_DIM, FI_ERR_INVALID, "ndim must be 1..%d (got %d)", FI_MAX_DIM, ndim);
	FI_REQUIRE(n >= 0 && num_clusters >= 0, FI_ERR_INVALID, "n = %ld, num_clusters = %ld", n, num_clusters);
	FI_REQUIRE(n == 0 || (positions != nullptr && labels != nullptr), FI_ERR_INVALID, "null positions or labels");
	FI_REQUIRE(num_clusters == 0 || rows != nullptr, FI_ERR_INVALID, "rows is null");
	fi::check_memory(memory);
	FI_REQUIRE(n < (1L << 31) && num_clusters < (1L << 31), FI_ERR_UNSUPPORTED, "%ld points, %ld clusters in one call", n, num_clusters);
	fi::cluster_measure(ndim, n, positions, labels, core, num_clusters, rows, memory);
	FI_API_END
}


// ---- the dominant hyperplanes of a point cloud (fi_plane.hip) -------------------------------------
namespace {
void check_plane(int ndim, long n, const float* positions, const fi_plane_options* opt, int memory)
{
	FI_REQUIRE(2 <= ndim && ndim <= FI_MAX_DIM, FI_ERR_INVALID, "ndim must be 2..%d (got %d)", FI_MAX_DIM, ndim);
	FI_REQUIRE(n >= 0, FI_ERR_INVALID, "n = %ld", n);
	FI_REQUIRE(n == 0 || positions != nullptr, FI_ERR_INVALID, "positions is null");
	FI_REQUIRE(opt != nullptr, FI_ERR_INVALID, "opt is null");
	FI_REQUIRE(opt->threshold >= 0.0f && !std::isinf(opt->threshold), FI_ERR_INVALID, "threshold must be finite and >= 0 (got %g)",
	           static_cast<double>(opt->threshold));  // (NaN fails)
	FI_REQUIRE(1 <= opt->max_trials && opt->max_trials <= (1L << 20), FI_ERR_INVALID, "max_trials must be 1..2^20 (got %ld)", opt->max_trials);
	FI_REQUIRE(opt->confidence >= 0.0 && opt->confidence < 1.0, FI_ERR_INVALID, "confidence must be in [0, 1) (got %g)", opt->confidence);
	FI_REQUIRE(0 <= opt->refine && opt->refine <= 16, FI_ERR_INVALID, "refine must be 0..16 (got %d)", opt->refine);
	FI_REQUIRE(opt->min_cos >= 0.0f && opt->min_cos <= 1.0f, FI_ERR_INVALID, "min_cos must be in [0, 1] (got %g)",
	           static_cast<double>(opt->min_cos));
	if (opt->min_cos > 0.0f) {
		bool finite = true, zero = true;
		for (int d = 0; d < ndim; ++d) {
			finite = finite && std::isfinite(opt->axis[d]);
			zero   = zero && opt->axis[d] == 0.0f;
		}
		FI_REQUIRE(finite && !zero, FI_ERR_INVALID, "min_cos > 0 needs a finite axis that is not zero");
	}
	fi::check_memory(memory);
}
}  // namespace

int fi_plane_fit(int ndim, long n, const float* positions, const unsigned char* mask, const fi_plane_options* opt, fi_plane_model* model,
                 unsigned char* inliers, int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(model != nullptr, FI_ERR_INVALID, "model is null");
	*model = fi_plane_model{};
	check_plane(ndim, n, positions, opt, memory);
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld points in one call", n);
	fi::plane_fit(ndim, n, positions, mask, *opt, model, inliers, memory);
	FI_API_END
}

int fi_planes_segment(int ndim, long n, const float* positions, const unsigned char* mask, const fi_plane_options* opt, int max_planes,
                      long min_inliers, int* labels, fi_plane_model* rows, int* num_planes, int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(num_planes != nullptr, FI_ERR_INVALID, "num_planes is null");
	*num_planes = 0;
	check_plane(ndim, n, positions, opt, memory);
	FI_REQUIRE(max_planes >= 1, FI_ERR_INVALID, "max_planes must be >= 1 (got %d)", max_planes);
	FI_REQUIRE(min_inliers >= 0, FI_ERR_INVALID, "min_inliers must be >= 0 (got %ld)", min_inliers);
	FI_REQUIRE(rows != nullptr && (n == 0 || labels != nullptr), FI_ERR_INVALID, "null labels or rows");
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld points in one call", n);
	fi::planes_segment(ndim, n, positions, mask, *opt, max_planes, min_inliers, labels, rows, num_planes, memory);
	FI_API_END
}


// ---- the spheres and cylinders of a point cloud (fi_shape.hip) ------------------------------------
namespace {
void check_shape(int ndim, long n, const float* positions, const float* normals, const fi_shape_options* opt, int memory)
{
	FI_REQUIRE(2 <= ndim && ndim <= FI_MAX_DIM, FI_ERR_INVALID, "ndim must be 2..%d (got %d)", FI_MAX_DIM, ndim);
	FI_REQUIRE(n >= 0, FI_ERR_INVALID, "n = %ld", n);
	FI_REQUIRE(n == 0 || positions != nullptr, FI_ERR_INVALID, "positions is null");
	FI_REQUIRE(opt != nullptr, FI_ERR_INVALID, "opt is null");
	FI_REQUIRE(opt->kind == FI_SHAPE_SPHERE || opt->kind == FI_SHAPE_CYLINDER, FI_ERR_INVALID, "unknown shape kind %d", opt->kind);
	FI_REQUIRE(opt->kind != FI_SHAPE_CYLINDER || ndim == 3, FI_ERR_UNSUPPORTED, "a cylinder needs ndim = 3 (got %d)", ndim);
	FI_REQUIRE(opt->kind != FI_SHAPE_CYLINDER || n == 0 || normals != nullptr, FI_ERR_INVALID, "a cylinder needs normals");
	FI_REQUIRE(opt->threshold >= 0.0f && !std::isinf(opt->threshold), FI_ERR_INVALID, "threshold must be finite and >= 0 (got %g)",
	           static_cast<double>(opt->threshold));  // (NaN fails)
	FI_REQUIRE(opt->r_min >= 0.0f && opt->r_max >= opt->r_min, FI_ERR_INVALID, "the radius limits must be 0 <= r_min <= r_max (got %g, %g)",
	           static_cast<double>(opt->r_min), static_cast<double>(opt->r_max));  // (a NaN fails)
	FI_REQUIRE(opt->normal_cos >= 0.0f && opt->normal_cos <= 1.0f, FI_ERR_INVALID, "normal_cos must be in [0, 1] (got %g)",
	           static_cast<double>(opt->normal_cos));
	FI_REQUIRE(!(opt->normal_cos > 0.0f) || n == 0 || normals != nullptr, FI_ERR_INVALID, "normal_cos > 0 needs normals");
	FI_REQUIRE(1 <= opt->max_trials && opt->max_trials <= (1L << 20), FI_ERR_INVALID, "max_trials must be 1..2^20 (got %ld)", opt->max_trials);
	FI_REQUIRE(opt->confidence >= 0.0 && opt->confidence < 1.0, FI_ERR_INVALID, "confidence must be in [0, 1) (got %g)", opt->confidence);
	FI_REQUIRE(0 <= opt->refine && opt->refine <= 16, FI_ERR_INVALID, "refine must be 0..16 (got %d)", opt->refine);
	fi::check_memory(memory);
}
}  // namespace

int fi_shape_fit(int ndim, long n, const float* positions, const float* normals, const unsigned char* mask, const fi_shape_options* opt,
                 fi_shape_model* model, unsigned char* inliers, int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(model != nullptr, FI_ERR_INVALID, "model is null");
	*model = fi_shape_model{};
	check_shape(ndim, n, positions, normals, opt, memory);
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld points in one call", n);
	fi::shape_fit(ndim, n, positions, normals, mask, *opt, model, inliers, memory);
	FI_API_END
}

int fi_shapes_segment(int ndim, long n, const float* positions, const float* normals, const unsigned char* mask, const fi_shape_options* opt,
                      int max_shapes, long min_inliers, int* labels, fi_shape_model* rows, int* num_shapes, int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(num_shapes != nullptr, FI_ERR_INVALID, "num_shapes is null");
	*num_shapes = 0;
	check_shape(ndim, n, positions, normals, opt, memory);
	FI_REQUIRE(max_shapes >= 1, FI_ERR_INVALID, "max_shapes must be >= 1 (got %d)", max_shapes);
	FI_REQUIRE(min_inliers >= 0, FI_ERR_INVALID, "min_inliers must be >= 0 (got %ld)", min_inliers);
	FI_REQUIRE(rows != nullptr && (n == 0 || labels != nullptr), FI_ERR_INVALID, "null labels or rows");
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld points in one call", n);
	fi::shapes_segment(ndim, n, positions, normals, mask, *opt, max_shapes, min_inliers, labels, rows, num_shapes, memory);
	FI_API_END
}


// ---- the rigid motion most matched pairs agree on (fi_align.hip) ----------------------------------
int fi_align_correspondences(long n_s, const float* source, long n_t, const float* target, long m, const long long* src_index,
                             const long long* tgt_index, const fi_align_options* opt, fi_alignment* out, unsigned char* inliers, int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "out is null");
	*out = fi_alignment{};
	for (int d = 0; d < 4; ++d) { out->transform[5 * d] = 1.0; }
	FI_REQUIRE(n_s >= 0 && n_t >= 0 && m >= 0, FI_ERR_INVALID, "n_s = %ld, n_t = %ld, m = %ld", n_s, n_t, m);
	FI_REQUIRE(opt != nullptr, FI_ERR_INVALID, "opt is null");
	FI_REQUIRE(opt->threshold >= 0.0f, FI_ERR_INVALID, "threshold must be >= 0 (got %g)", static_cast<double>(opt->threshold));  // (NaN fails)
	FI_REQUIRE(opt->similarity >= 0.0f && opt->similarity <= 1.0f, FI_ERR_INVALID, "similarity must be in [0, 1] (got %g)",
	           static_cast<double>(opt->similarity));
	FI_REQUIRE(opt->confidence >= 0.0 && opt->confidence < 1.0, FI_ERR_INVALID, "confidence must be in [0, 1) (got %g)", opt->confidence);
	FI_REQUIRE(1 <= opt->max_trials && opt->max_trials <= 0x7FFFFFFFL, FI_ERR_INVALID, "max_trials must be 1..2^31 - 1 (got %ld)",
	           opt->max_trials);
	fi::check_memory(memory);
	FI_REQUIRE(m == 0 || (src_index != nullptr && tgt_index != nullptr), FI_ERR_INVALID, "null indices");
	FI_REQUIRE(m == 0 || ((n_s == 0 || source != nullptr) && (n_t == 0 || target != nullptr)), FI_ERR_INVALID, "null points");
	FI_REQUIRE(m < (1L << 31) && n_s < (1L << 31) && n_t < (1L << 31), FI_ERR_UNSUPPORTED, "%ld pairs over %ld and %ld points in one call", m,
	           n_s, n_t);
	fi::align_correspondences(n_s, source, n_t, target, m, src_index, tgt_index, *opt, out, inliers, memory);
	FI_API_END
}


// ---- descriptors of a point's neighbourhood and their matching (fi_feature.hip) --------------------
int fi_points_describe(fi_points* h, const float* normals, int k, float max_distance, float* features, unsigned char* valid, int memory)
{
	FI_API_BEGIN
	check_points(h);
	check_k(k);
	FI_REQUIRE(normals != nullptr && features != nullptr, FI_ERR_INVALID, "null normals or features");
	FI_REQUIRE(max_distance >= 0.0f, FI_ERR_INVALID, "max_distance must be >= 0 (got %g)", static_cast<double>(max_distance));  // (NaN fails)
	fi::check_memory(memory);
	FI_REQUIRE(h->t.D == 3, FI_ERR_UNSUPPORTED, "descriptors need 3 dimensions (the set has %d)", h->t.D);
	fi::points_describe(h->t, normals, k, max_distance, features, valid, memory, nullptr);
	FI_API_END
}

int fi_feature_match(int dim, long n_a, const float* a, const unsigned char* valid_a, long n_b, const float* b, const unsigned char* valid_b,
                     long long* indices, float* distances, int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(1 <= dim && dim <= FI_FEATURE_MAX_DIM, FI_ERR_INVALID, "dim must be 1..%d (got %d)", FI_FEATURE_MAX_DIM, dim);
	FI_REQUIRE(n_a >= 0 && n_b >= 0, FI_ERR_INVALID, "n_a = %ld, n_b = %ld", n_a, n_b);
	FI_REQUIRE(n_a == 0 || (a != nullptr && indices != nullptr), FI_ERR_INVALID, "null a or indices");
	FI_REQUIRE(n_a == 0 || n_b == 0 || b != nullptr, FI_ERR_INVALID, "b is null");
	fi::check_memory(memory);
	FI_REQUIRE(n_a < (1L << 31) && n_b < (1L << 31), FI_ERR_UNSUPPORTED, "%ld rows against %ld in one call", n_a, n_b);
	fi::feature_match(dim, n_a, a, valid_a, n_b, b, valid_b, indices, distances, memory);
	FI_API_END
}


// ---- a consistent sign for normals (fi_orient.hip) ----------------------------------------------
namespace {
int points_orient_normals(PointSet s, int k, float max_distance, int anchor, const float* guides, long num_guides, float* normals,
                          long long* components, int memory)
{
	FI_API_BEGIN
	s.bind();
	check_normals("anchor", false, s.ndim(), k, max_distance, anchor, normals, memory);
	s.whole();
	const fi::NearestIndex& t = s.index();
	check_guides("anchor", t, anchor, guides, num_guides);
	fi::orient_normals(t, k, max_distance, anchor, guides, num_guides, normals, components, memory, s.stream());
	FI_API_END
}
}  // namespace

int fi_orient_normals(fi_ctx* c, int k, float max_distance, int anchor, const float* guides, long num_guides, float* normals,
                      long long* components, int memory)
{
	return points_orient_normals(c, k, max_distance, anchor, guides, num_guides, normals, components, memory);
}

int fi_points_orient_normals(fi_points* h, int k, float max_distance, int anchor, const float* guides, long num_guides,
                             float* normals, long long* components, int memory)
{
	return points_orient_normals(h, k, max_distance, anchor, guides, num_guides, normals, components, memory);
}


// ---- distances to a surface; redistancing (fi_surface.hip) -------------------------------------
namespace {
void check_surface(const fi_surface* h)
{
	FI_REQUIRE(h != nullptr, FI_ERR_INVALID, "surface is null");
	FI_HIP_TRY(hipSetDevice(h->device));
}

void check_redistance(int method, float max_distance, const float* out, int memory)
{
	FI_REQUIRE(method == FI_SURFACE_ISO || method == FI_SURFACE_DUAL, FI_ERR_INVALID, "unknown surface method %d", method);
	check_field_out(max_distance, out, memory);
}
}  // namespace

int fi_surface_create(fi_surface** out, int ndim, long num_vertices, const float* vertices, long num_primitives, const int* indices,
                      int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "out is null");
	*out = nullptr;
	FI_REQUIRE(ndim == 2 || ndim == 3, FI_ERR_UNSUPPORTED, "surfaces in %d-D are not supported (2-D segments, 3-D triangles)", ndim);
	FI_REQUIRE(num_vertices >= 0 && num_primitives >= 0, FI_ERR_INVALID, "%ld vertices, %ld primitives", num_vertices, num_primitives);
	FI_REQUIRE(num_vertices == 0 || vertices != nullptr, FI_ERR_INVALID, "vertices is null");
	FI_REQUIRE(num_primitives == 0 || indices != nullptr, FI_ERR_INVALID, "indices is null");
	fi::check_memory(memory);
	FI_REQUIRE(num_primitives < (1L << 31), FI_ERR_UNSUPPORTED, "%ld primitives: primitive indices are 32-bit", num_primitives);
	std::unique_ptr<fi_surface> h(new fi_surface());
	FI_HIP_TRY(hipGetDevice(&h->device));
	fi::stage::In<float> v(num_vertices > 0 ? vertices : nullptr, static_cast<int64_t>(ndim) * num_vertices, memory, nullptr);
	fi::stage::In<int>   i(num_primitives > 0 ? indices : nullptr, static_cast<int64_t>(ndim) * num_primitives, memory, nullptr);
	fi::surface_build(h->t, ndim, num_vertices, v, num_primitives, i, nullptr);
	*out = h.release();
	FI_API_END
}

int fi_surface_from_mesh(fi_surface** out, const fi_mesh* mesh)
{
	FI_API_BEGIN
	FI_REQUIRE(out != nullptr && mesh != nullptr, FI_ERR_INVALID, "null argument");
	*out = nullptr;
	FI_HIP_TRY(hipSetDevice(mesh->device));
	std::unique_ptr<fi_surface> h(new fi_surface());
	h->device = mesh->device;
	fi::surface_build(h->t, mesh->ndim, mesh->nv, mesh->pos.as<float>(), mesh->np, mesh->idx.as<int>(), nullptr);
	*out = h.release();
	FI_API_END
}

int fi_surface_distance(fi_surface* h, long n, const float* queries, float max_distance, float* distances, long long* primitives,
                        float* closest, int memory)
{
	FI_API_BEGIN
	check_surface(h);
	check_nearest(n, queries, max_distance, distances, memory);
	fi::surface_query(h->t, n, queries, max_distance, distances, primitives, closest, memory, nullptr);
	FI_API_END
}

int fi_surface_distance_field(fi_surface* h, const int* sizes, float max_distance, float* out, long long* primitives, int memory)
{
	FI_API_BEGIN
	check_surface(h);
	FI_REQUIRE(sizes != nullptr, FI_ERR_INVALID, "sizes is null");
	for (int d = 0; d < h->t.D; ++d) { FI_REQUIRE(sizes[d] >= 1, FI_ERR_INVALID, "sizes[%d] = %d", d, sizes[d]); }
	check_field_out(max_distance, out, memory);
	fi::surface_lattice(h->t, sizes, max_distance, out, primitives, memory, nullptr);
	FI_API_END
}

int fi_surface_destroy(fi_surface* h) { return fi::destroy_handle(h); }

// ---- rays against a surface (fi_ray.hip) ---------------------------------------------------------
namespace {
void check_rays(long n, const float* origins, const float* directions, float t_min, float t_max, const void* out, int memory)
{
	FI_REQUIRE(n >= 0, FI_ERR_INVALID, "n = %ld", n);
	FI_REQUIRE(origins != nullptr && directions != nullptr && out != nullptr, FI_ERR_INVALID, "null origins, directions or output");
	FI_REQUIRE(t_min <= t_max, FI_ERR_INVALID, "t_min = %g, t_max = %g", static_cast<double>(t_min), static_cast<double>(t_max));  // (NaN fails)
	fi::check_memory(memory);
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld rays in one call", n);
}
}  // namespace

int fi_surface_raycast(fi_surface* h, long n, const float* origins, const float* directions, float t_min, float t_max, float* t,
                       long long* primitives, float* bary, int memory)
{
	FI_API_BEGIN
	check_surface(h);
	check_rays(n, origins, directions, t_min, t_max, t, memory);
	fi::ray_cast(h->t, n, origins, directions, t_min, t_max, t, primitives, bary, memory, nullptr);
	FI_API_END
}

int fi_surface_count_hits(fi_surface* h, long n, const float* origins, const float* directions, float t_min, float t_max, int limit,
                          int* counts, int memory)
{
	FI_API_BEGIN
	check_surface(h);
	check_rays(n, origins, directions, t_min, t_max, counts, memory);
	FI_REQUIRE(limit >= 1, FI_ERR_INVALID, "limit = %d", limit);
	fi::ray_count(h->t, n, origins, directions, t_min, t_max, limit, counts, memory, nullptr);
	FI_API_END
}

int fi_surface_contains(fi_surface* h, long n, const float* points, const float* direction, unsigned char* inside, int memory)
{
	FI_API_BEGIN
	check_surface(h);
	check_rays(n, points, points, 0.0f, INFINITY, inside, memory);
	fi::ray_contains(h->t, n, points, direction, inside, memory, nullptr);
	FI_API_END
}

int fi_surface_signed_distance(fi_surface* h, long n, const float* queries, float max_distance, float* distances,
                               long long* primitives, float* closest, int memory)
{
	FI_API_BEGIN
	check_surface(h);
	check_nearest(n, queries, max_distance, distances, memory);
	fi::ray_signed_query(h->t, n, queries, max_distance, distances, primitives, closest, memory, nullptr);
	FI_API_END
}

int fi_surface_signed_distance_field(fi_surface* h, const int* sizes, float max_distance, float* out, long long* primitives,
                                     int memory)
{
	FI_API_BEGIN
	check_surface(h);
	FI_REQUIRE(sizes != nullptr, FI_ERR_INVALID, "sizes is null");
	for (int d = 0; d < h->t.D; ++d) { FI_REQUIRE(sizes[d] >= 1, FI_ERR_INVALID, "sizes[%d] = %d", d, sizes[d]); }
	check_field_out(max_distance, out, memory);
	fi::ray_signed_lattice(h->t, sizes, max_distance, out, primitives, memory, nullptr);
	FI_API_END
}

int fi_redistance(fi_ctx* c, const float* field, float iso, int method, float max_distance, float* out, long long* primitives,
                  fi_mesh** mesh, int memory)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	if (mesh) { *mesh = nullptr; }
	fi::bind_device(c);
	check_redistance(method, max_distance, out, memory);
	fi::redistance_ctx(c, field, iso, method, max_distance, out, primitives, mesh, memory);
	FI_API_END
}

int fi_redistance_field(const float* field, int ndim, const int* sizes, float iso, int method, float max_distance, float* out,
                        long long* primitives, fi_mesh** mesh, int memory)
{
	FI_API_BEGIN
	if (mesh) { *mesh = nullptr; }
	FI_REQUIRE(field && sizes, FI_ERR_INVALID, "null argument");
	check_redistance(method, max_distance, out, memory);
	FI_REQUIRE(ndim == 2 || ndim == 3, FI_ERR_UNSUPPORTED, "redistancing a %d-D lattice is not supported", ndim);
	const int64_t n = fi::lattice_points(ndim, sizes);
	FI_REQUIRE(n < (int64_t(1) << 31), FI_ERR_UNSUPPORTED, "a lattice of %lld points", static_cast<long long>(n));
	fi::stage::In<float> f(field, n, memory, nullptr);
	fi::redistance_whole(f, ndim, sizes, iso, method, max_distance, out, primitives, mesh, memory, nullptr);
	FI_API_END
}

// ---- depth images: oriented points, and a truncated signed distance volume (fi_depth.hip) -----------
namespace {
void check_volume(const fi_volume* v)
{
	FI_REQUIRE(v != nullptr, FI_ERR_INVALID, "volume is null");
	FI_HIP_TRY(hipSetDevice(v->device));
}

// the cameras of a call and the pixels of their images together
int64_t check_cameras(long m, const fi_camera* cameras)
{
	FI_REQUIRE(m >= 0, FI_ERR_INVALID, "m = %ld", m);
	FI_REQUIRE(m == 0 || cameras != nullptr, FI_ERR_INVALID, "cameras is null");
	int64_t pixels = 0;
	for (long s = 0; s < m; ++s) {
		fi::check_camera(cameras[s]);
		pixels += fi::camera_pixels(cameras[s]);
		FI_REQUIRE(pixels < (int64_t(1) << 31), FI_ERR_UNSUPPORTED, "more than 2^31 - 1 pixels in one call");
	}
	return pixels;
}
}  // namespace

int fi_depth_unproject(const fi_camera* camera, const float* depth, float max_jump, float* positions, float* normals, float* incidence,
                       unsigned char* valid, int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(camera != nullptr && depth != nullptr, FI_ERR_INVALID, "null camera or depth");
	FI_REQUIRE(max_jump >= 0.0f, FI_ERR_INVALID, "max_jump must be >= 0 (got %g)", static_cast<double>(max_jump));  // (NaN fails)
	FI_REQUIRE(positions || normals || incidence || valid, FI_ERR_INVALID, "every output is null");
	fi::check_memory(memory);
	check_cameras(1, camera);
	fi::depth_unproject(*camera, depth, max_jump, positions, normals, incidence, valid, memory, nullptr);
	FI_API_END
}

int fi_volume_create(fi_volume** out, int ndim, const int* sizes, float truncation, float max_weight)
{
	FI_API_BEGIN
	FI_REQUIRE(out != nullptr, FI_ERR_INVALID, "out is null");
	*out = nullptr;
	FI_REQUIRE(1 <= ndim && ndim <= FI_MAX_DIM && sizes != nullptr, FI_ERR_INVALID, "ndim must be 1..%d with sizes (got %d)", FI_MAX_DIM, ndim);
	const int64_t n = fi::lattice_points(ndim, sizes);
	FI_REQUIRE(truncation > 0.0f && std::isfinite(truncation), FI_ERR_INVALID, "truncation must be > 0 and finite (got %g)",
	           static_cast<double>(truncation));
	FI_REQUIRE(max_weight > 0.0f, FI_ERR_INVALID, "max_weight must be > 0 (got %g)", static_cast<double>(max_weight));  // (NaN fails)
	FI_REQUIRE(ndim == 3, FI_ERR_UNSUPPORTED, "a volume over a %d-D lattice is not supported", ndim);
	FI_REQUIRE(n < (int64_t(1) << 31), FI_ERR_UNSUPPORTED, "a volume of %lld voxels", static_cast<long long>(n));
	std::unique_ptr<fi_volume> v(new fi_volume());
	FI_HIP_TRY(hipGetDevice(&v->device));
	for (int d = 0; d < 3; ++d) { v->n[d] = sizes[d]; }
	v->nvox       = n;
	v->truncation = truncation;
	v->max_weight = max_weight;
	v->tsdf.alloc(sizeof(float) * n);
	v->weight.alloc(sizeof(float) * n);
	fi::volume_reset(v.get(), nullptr);
	*out = v.release();
	FI_API_END
}

int fi_volume_destroy(fi_volume* v) { return fi::destroy_handle(v); }

int fi_volume_load(fi_volume* v, const float* tsdf, const float* weight, int memory)
{
	FI_API_BEGIN
	check_volume(v);
	FI_REQUIRE(tsdf != nullptr && weight != nullptr, FI_ERR_INVALID, "null tsdf or weight");
	fi::check_memory(memory);
	const hipMemcpyKind kind = memory == FI_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
	FI_HIP_TRY(hipMemcpyAsync(v->tsdf.p, tsdf, sizeof(float) * v->nvox, kind, nullptr));
	FI_HIP_TRY(hipMemcpyAsync(v->weight.p, weight, sizeof(float) * v->nvox, kind, nullptr));
	FI_HIP_TRY(hipStreamSynchronize(nullptr));
	FI_API_END
}

int fi_volume_copy(const fi_volume* v, float* tsdf, float* weight, int memory)
{
	FI_API_BEGIN
	check_volume(v);
	FI_REQUIRE(tsdf != nullptr || weight != nullptr, FI_ERR_INVALID, "null tsdf and weight");
	fi::check_memory(memory);
	const hipMemcpyKind kind = memory == FI_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
	if (tsdf) { FI_HIP_TRY(hipMemcpyAsync(tsdf, v->tsdf.p, sizeof(float) * v->nvox, kind, nullptr)); }
	if (weight) { FI_HIP_TRY(hipMemcpyAsync(weight, v->weight.p, sizeof(float) * v->nvox, kind, nullptr)); }
	FI_HIP_TRY(hipStreamSynchronize(nullptr));
	FI_API_END
}

int fi_volume_integrate(fi_volume* v, long m, const fi_camera* cameras, const float* depths, const float* incidences,
                        const float* image_weights, float min_incidence, int memory)
{
	FI_API_BEGIN
	check_volume(v);
	FI_REQUIRE(min_incidence == min_incidence, FI_ERR_INVALID, "min_incidence is NaN");
	fi::check_memory(memory);
	check_cameras(m, cameras);
	FI_REQUIRE(m == 0 || depths != nullptr, FI_ERR_INVALID, "depths is null");
	fi::volume_integrate(v, m, cameras, depths, incidences, image_weights, min_incidence, memory, nullptr);
	FI_API_END
}

int fi_volume_constraints(const fi_volume* v, float min_weight, long* n, float* positions, float* values, float* weights, int memory)
{
	FI_API_BEGIN
	check_volume(v);
	FI_REQUIRE(n != nullptr, FI_ERR_INVALID, "n is null");
	FI_REQUIRE(min_weight == min_weight, FI_ERR_INVALID, "min_weight is NaN");
	fi::check_memory(memory);
	const bool fill = positions || values || weights;
	FI_REQUIRE(!fill || *n >= 0, FI_ERR_INVALID, "room for %ld points", *n);
	*n = static_cast<long>(fi::volume_constraints(v, min_weight, fill ? *n : 0, positions, values, weights, memory, nullptr));
	FI_API_END
}

int fi_add_volume(fi_ctx* c, const fi_volume* v, float value_weight, int value_kernel, float min_weight)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	fi::bind_device(c);
	FI_REQUIRE(v != nullptr, FI_ERR_INVALID, "volume is null");
	FI_REQUIRE(value_kernel == FI_VALUE_NEAREST_NEIGHBOR || value_kernel == FI_VALUE_LINEAR_INTERPOLATION, FI_ERR_INVALID,
	           "Unknown value kernel: %d", value_kernel);
	FI_REQUIRE(min_weight == min_weight, FI_ERR_INVALID, "min_weight is NaN");
	FI_REQUIRE(c->g.ndim == 3, FI_ERR_UNSUPPORTED, "a volume into a %d-D lattice is not supported", c->g.ndim);
	FI_REQUIRE(c->nranks == 1, FI_ERR_UNSUPPORTED, "fi_add_volume on a slab context: the volume covers the whole lattice");
	FI_REQUIRE(c->g.gn[0] == v->n[0] && c->g.gn[1] == v->n[1] && c->g.gn[2] == v->n[2], FI_ERR_INVALID,
	           "the volume is %d x %d x %d, the lattice %d x %d x %d", v->n[0], v->n[1], v->n[2], c->g.gn[0], c->g.gn[1], c->g.gn[2]);
	FI_REQUIRE(c->device == v->device, FI_ERR_INVALID, "the volume lives on device %d, the context on %d", v->device, c->device);
	fi::DevBuf    pos, val, wgt, zero;
	const int64_t n = fi::volume_constraints_device(v, min_weight, pos, val, wgt, c->stream);
	if (n == 0) { return FI_OK; }
	const float* nrm = nullptr;
	if (value_kernel == FI_VALUE_NEAREST_NEIGHBOR) {
		// that kernel's row reads the point's gradient for the step to its lattice point: zero here, as the step is
		zero.alloc(sizeof(float) * 3 * n);
		FI_HIP_TRY(hipMemsetAsync(zero.p, 0, sizeof(float) * 3 * n, c->stream));
		nrm = zero.as<float>();
	}
	fi::nearest_release(c);  // (a new point set)
	fi::add_points_device(c, static_cast<long>(n), pos.as<float>(), nrm, wgt.as<float>(), val.as<float>(), value_weight, value_kernel, 0.0f,
	                      FI_GRADIENT_NEAREST_NEIGHBOR);
	c->assembled = false;
	FI_API_END
}

// ---- rays and pinhole images of a lattice field or a depth volume (fi_march.hip) ---------------------
namespace {
void check_march_rays(const fi_march_options* options, long n, const float* origins, const float* directions, float t_min, float t_max,
                      const float* t, const float* positions, const float* normals, const signed char* side, int memory)
{
	fi::check_march_options(options);
	FI_REQUIRE(n >= 0, FI_ERR_INVALID, "n = %ld", n);
	FI_REQUIRE(n == 0 || (origins != nullptr && directions != nullptr), FI_ERR_INVALID, "null origins or directions");
	FI_REQUIRE(t || positions || normals || side, FI_ERR_INVALID, "every output is null");
	FI_REQUIRE(t_min <= t_max, FI_ERR_INVALID, "t_min = %g, t_max = %g", static_cast<double>(t_min), static_cast<double>(t_max));  // (NaN fails)
	fi::check_memory(memory);
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld rays in one call", n);
}

void check_march_image(const fi_march_options* options, const fi_camera* camera, const float* depth, int memory)
{
	fi::check_march_options(options);
	FI_REQUIRE(camera != nullptr && depth != nullptr, FI_ERR_INVALID, "null camera or depth");
	fi::check_memory(memory);
	check_cameras(1, camera);
}

fi::MarchField march_field(const float* f, const float* w, int ndim, const int* sizes)
{
	fi::MarchField m{f, w, ndim, {1, 1, 1}};
	for (int d = 0; d < ndim; ++d) { m.n[d] = sizes[d]; }
	return m;
}

// the lattice field of an undivided context on its device: the caller's values, or its last solution (buf: an fp32 copy)
fi::MarchField march_ctx_field(fi_ctx* c, const float* field, int memory, fi::DevBuf& buf)
{
	FI_REQUIRE(c->nranks == 1, FI_ERR_UNSUPPORTED, "rays against the field of a slab context are not supported");
	fi::check_march_field(c->g.ndim, c->g.gn);
	FI_REQUIRE(field || c->vectors_ready, FI_ERR_STATE, "no solution yet");
	return march_field(fi::field_f32(c, field, memory, buf), nullptr, c->g.ndim, c->g.gn);
}
}  // namespace

int fi_march_default_options(fi_march_options* options)
{
	FI_API_BEGIN
	FI_REQUIRE(options != nullptr, FI_ERR_INVALID, "options is null");
	*options = fi_march_options{0.0f, 1.0f, 0.0f, 4, FI_MARCH_FRONT};
	FI_API_END
}

int fi_field_raycast(const float* field, const float* weight, int ndim, const int* sizes, const fi_march_options* options, long n,
                     const float* origins, const float* directions, float t_min, float t_max, float* t, float* positions,
                     float* normals, signed char* side, int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(field != nullptr, FI_ERR_INVALID, "field is null");
	check_march_rays(options, n, origins, directions, t_min, t_max, t, positions, normals, side, memory);
	const int64_t total = fi::check_march_field(ndim, sizes);
	if (n == 0) { return FI_OK; }
	fi::stage::In<float> f(field, total, memory, nullptr), w(weight, total, memory, nullptr);
	fi::march_rays(march_field(f, w, ndim, sizes), *options, n, origins, directions, t_min, t_max, t, positions, normals, side, memory,
	               nullptr);
	FI_API_END
}

int fi_field_render(const float* field, const float* weight, const int* sizes, const fi_march_options* options,
                    const fi_camera* camera, float* depth, float* positions, float* normals, float* incidence, int memory)
{
	FI_API_BEGIN
	FI_REQUIRE(field != nullptr, FI_ERR_INVALID, "field is null");
	check_march_image(options, camera, depth, memory);
	const int64_t total = fi::check_march_field(3, sizes);
	fi::stage::In<float> f(field, total, memory, nullptr), w(weight, total, memory, nullptr);
	fi::march_image(march_field(f, w, 3, sizes), *options, *camera, depth, positions, normals, incidence, memory, nullptr);
	FI_API_END
}

int fi_raycast_field(fi_ctx* c, const float* field, const fi_march_options* options, long n, const float* origins,
                     const float* directions, float t_min, float t_max, float* t, float* positions, float* normals, signed char* side,
                     int memory)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	fi::bind_device(c);
	check_march_rays(options, n, origins, directions, t_min, t_max, t, positions, normals, side, memory);
	fi::AllocStream      alloc_on(c->stream);
	fi::DevBuf           buf;
	const fi::MarchField f = march_ctx_field(c, field, memory, buf);
	fi::march_rays(f, *options, n, origins, directions, t_min, t_max, t, positions, normals, side, memory, c->stream);
	FI_HIP_TRY(hipStreamSynchronize(c->stream));  // (n = 0: the copy into buf ends before buf goes)
	FI_API_END
}

int fi_render_field(fi_ctx* c, const float* field, const fi_march_options* options, const fi_camera* camera, float* depth,
                    float* positions, float* normals, float* incidence, int memory)
{
	FI_API_BEGIN
	fi::check_ctx(c);
	fi::bind_device(c);
	check_march_image(options, camera, depth, memory);
	FI_REQUIRE(c->g.ndim != 2, FI_ERR_UNSUPPORTED, "an image of a 2-D field is not supported");
	fi::AllocStream      alloc_on(c->stream);
	fi::DevBuf           buf;
	const fi::MarchField f = march_ctx_field(c, field, memory, buf);
	fi::march_image(f, *options, *camera, depth, positions, normals, incidence, memory, c->stream);
	FI_API_END
}

int fi_volume_raycast(const fi_volume* v, const fi_march_options* options, long n, const float* origins, const float* directions,
                      float t_min, float t_max, float* t, float* positions, float* normals, signed char* side, int memory)
{
	FI_API_BEGIN
	check_volume(v);
	check_march_rays(options, n, origins, directions, t_min, t_max, t, positions, normals, side, memory);
	fi::check_march_field(3, v->n);
	fi::march_rays(march_field(v->tsdf.as<float>(), v->weight.as<float>(), 3, v->n), *options, n, origins, directions, t_min, t_max, t,
	               positions, normals, side, memory, nullptr);
	FI_API_END
}

int fi_volume_render(const fi_volume* v, const fi_march_options* options, const fi_camera* camera, float* depth, float* positions,
                     float* normals, float* incidence, int memory)
{
	FI_API_BEGIN
	check_volume(v);
	check_march_image(options, camera, depth, memory);
	fi::check_march_field(3, v->n);
	fi::march_image(march_field(v->tsdf.as<float>(), v->weight.as<float>(), 3, v->n), *options, *camera, depth, positions, normals,
	                incidence, memory, nullptr);
	FI_API_END
}

// ---- colour in a depth volume (fi_colour.hip) ---------------------------------------------------------
namespace {
void check_coloured(const fi_volume* v)
{
	check_volume(v);
	FI_REQUIRE(v->channels > 0, FI_ERR_STATE, "the volume has no colour channels (fi_volume_set_channels)");
}

// sampling reads the eight corners of a cell
void check_colour_cells(const fi_volume* v)
{
	FI_REQUIRE(v->n[0] >= 2 && v->n[1] >= 2 && v->n[2] >= 2, FI_ERR_UNSUPPORTED, "colour sampling needs sizes >= 2 (a %d x %d x %d volume)",
	           v->n[0], v->n[1], v->n[2]);
}
}  // namespace

int fi_volume_set_channels(fi_volume* v, int channels)
{
	FI_API_BEGIN
	check_volume(v);
	FI_REQUIRE(channels >= 1 && channels <= fi::kMaxChannels, FI_ERR_INVALID, "channels must be 1..%d (got %d)", fi::kMaxChannels, channels);
	FI_REQUIRE(v->channels == 0, FI_ERR_STATE, "the volume has %d channels already", v->channels);
	fi::volume_set_channels(v, channels, nullptr);
	FI_API_END
}

int fi_volume_channels(const fi_volume* v, int* channels)
{
	FI_API_BEGIN
	FI_REQUIRE(v != nullptr && channels != nullptr, FI_ERR_INVALID, "null argument");
	*channels = v->channels;
	FI_API_END
}

int fi_volume_colour_load(fi_volume* v, const float* colour, const float* colour_weight, int memory)
{
	FI_API_BEGIN
	check_coloured(v);
	FI_REQUIRE(colour != nullptr && colour_weight != nullptr, FI_ERR_INVALID, "null colour or colour_weight");
	fi::check_memory(memory);
	const hipMemcpyKind kind = memory == FI_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
	FI_HIP_TRY(hipMemcpyAsync(v->colour.p, colour, sizeof(float) * v->channels * v->nvox, kind, nullptr));
	FI_HIP_TRY(hipMemcpyAsync(v->colour_weight.p, colour_weight, sizeof(float) * v->nvox, kind, nullptr));
	FI_HIP_TRY(hipStreamSynchronize(nullptr));
	FI_API_END
}

int fi_volume_colour_copy(const fi_volume* v, float* colour, float* colour_weight, int memory)
{
	FI_API_BEGIN
	check_coloured(v);
	FI_REQUIRE(colour != nullptr || colour_weight != nullptr, FI_ERR_INVALID, "null colour and colour_weight");
	fi::check_memory(memory);
	const hipMemcpyKind kind = memory == FI_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
	if (colour) { FI_HIP_TRY(hipMemcpyAsync(colour, v->colour.p, sizeof(float) * v->channels * v->nvox, kind, nullptr)); }
	if (colour_weight) { FI_HIP_TRY(hipMemcpyAsync(colour_weight, v->colour_weight.p, sizeof(float) * v->nvox, kind, nullptr)); }
	FI_HIP_TRY(hipStreamSynchronize(nullptr));
	FI_API_END
}

int fi_volume_integrate_colour(fi_volume* v, long m, const fi_camera* cameras, const float* depths, const float* incidences,
                               const float* image_weights, float min_incidence, const float* colours, float band, int memory)
{
	FI_API_BEGIN
	check_coloured(v);
	FI_REQUIRE(min_incidence == min_incidence, FI_ERR_INVALID, "min_incidence is NaN");
	FI_REQUIRE(band > 0.0f && band <= 1.0f, FI_ERR_INVALID, "band must be in (0, 1] (got %g)", static_cast<double>(band));  // (NaN fails)
	fi::check_memory(memory);
	check_cameras(m, cameras);
	FI_REQUIRE(m == 0 || depths != nullptr, FI_ERR_INVALID, "depths is null");
	FI_REQUIRE(m == 0 || colours != nullptr, FI_ERR_INVALID, "colours is null");
	fi::volume_integrate_colour(v, m, cameras, depths, incidences, image_weights, min_incidence, colours, band, memory, nullptr);
	FI_API_END
}

int fi_volume_colour_sample(const fi_volume* v, float min_weight, long n, const float* positions, float* colours, unsigned char* valid,
                            int memory)
{
	FI_API_BEGIN
	check_coloured(v);
	FI_REQUIRE(min_weight == min_weight, FI_ERR_INVALID, "min_weight is NaN");
	FI_REQUIRE(n >= 0, FI_ERR_INVALID, "n = %ld", n);
	FI_REQUIRE(n == 0 || positions != nullptr, FI_ERR_INVALID, "positions is null");
	FI_REQUIRE(n == 0 || colours != nullptr, FI_ERR_INVALID, "colours is null");
	fi::check_memory(memory);
	FI_REQUIRE(n < (1L << 31), FI_ERR_UNSUPPORTED, "%ld points in one call", n);
	check_colour_cells(v);
	fi::volume_colour_sample(v, min_weight, n, positions, colours, valid, memory, nullptr);
	FI_API_END
}

int fi_volume_render_colour(const fi_volume* v, const fi_march_options* options, const fi_camera* camera, float colour_min_weight,
                            float* depth, float* positions, float* normals, float* incidence, float* colours, int memory)
{
	FI_API_BEGIN
	check_coloured(v);
	check_march_image(options, camera, depth, memory);
	FI_REQUIRE(colour_min_weight == colour_min_weight, FI_ERR_INVALID, "colour_min_weight is NaN");
	FI_REQUIRE(colours != nullptr, FI_ERR_INVALID, "colours is null");
	check_colour_cells(v);
	fi::check_march_field(3, v->n);
	fi::volume_render_colour(v, *options, *camera, colour_min_weight, depth, positions, normals, incidence, colours, memory, nullptr);
	FI_API_END
}

int fi_volume_colour_constraints(const fi_volume* v, float min_weight, long* n, float* positions, float* colours, float* weights, int memory)
{
	FI_API_BEGIN
	check_coloured(v);
	FI_REQUIRE(n != nullptr, FI_ERR_INVALID, "n is null");
	FI_REQUIRE(min_weight == min_weight, FI_ERR_INVALID, "min_weight is NaN");
	fi::check_memory(memory);
	const bool fill = positions || colours || weights;
	FI_REQUIRE(!fill || *n >= 0, FI_ERR_INVALID, "room for %ld points", *n);
	*n = static_cast<long>(fi::volume_colour_constraints(v, min_weight, fill ? *n : 0, positions, colours, weights, memory, nullptr));
	FI_API_END
}

}  // extern "C"
