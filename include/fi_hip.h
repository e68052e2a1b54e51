/* fi_hip.h -- C ABI of the MI355X-native field_interpolation solver core (libfi_hip.so).
 *
 * This is the drop-in boundary: plain C, opaque context, POD structs, caller-owned buffers, integer
 * status codes, no exceptions, no aborts.  Everything above it (the C++ headers in
 * include/field_interpolation/, the ctypes mirror in field_interpolation_amd/) is host plumbing;
 * everything below it is hand-written HIP for gfx950.
 *
 * Each entry point names the reference interface it replaces (file:line under the reference tree,
 * emilk/field_interpolation).
 *
 * Conventions
 *   - all calls are synchronous: they return after the GPU work they started has completed;
 *   - `memory` says where caller buffers live: FI_HOST (malloc'ed) or FI_DEVICE (HBM pointers of the
 *     current device, e.g. torch tensor data_ptr(); the caller must have finished writing them);
 *   - positions / normals are interleaved xyzxyz... fp32 in LATTICE coordinates, exactly like
 *     field_interpolation.hpp:153-173;
 *   - a context is not thread safe; different contexts may be used from different threads.
 *   - return value 0 = FI_OK; otherwise fi_last_error() holds a message for the calling thread.
 */
#ifndef FI_HIP_H
#define FI_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define FI_OK 0
#define FI_ERR_INVALID 1      /* bad argument (the reference CHECK_F / ABORT_F cases) */
#define FI_ERR_HIP 2          /* HIP runtime failure */
#define FI_ERR_STATE 3        /* call order violated (e.g. solve before assemble) */
#define FI_ERR_COMM 4         /* RCCL failure */
#define FI_ERR_UNSUPPORTED 5  /* valid in the reference, not available in this mode */
#define FI_ERR_BREAKDOWN 6    /* solver breakdown (non-finite or non-positive curvature): reference returns {} */
#define FI_ERR_TIMEOUT 7      /* the wall-clock guard of a solve (FI_SOLVE_TIMEOUT_S, default 600 s) stopped it; over slabs
                                 all ranks stop in the same round.  The iterate is kept in the context. */

#define FI_HOST 0
#define FI_DEVICE 1

#define FI_F32 0 /* all vectors and operator coefficients fp32, reductions fp64 */
#define FI_F64 1 /* everything fp64 */

#define FI_MAX_DIM 3 /* field_interpolation.hpp:44 */

#define FI_SAMPLE_LINEAR 0 /* fi_sample*: multilinear (the reference's multilerp, field_interpolation.cpp:15-55) */
#define FI_SAMPLE_CUBIC 1  /* fi_sample*: Catmull-Rom with clamped indices (the SDF app's bicubic_upsample) */

/* field_interpolation.hpp:47-59 */
#define FI_VALUE_NEAREST_NEIGHBOR 0
#define FI_VALUE_LINEAR_INTERPOLATION 1
#define FI_GRADIENT_NEAREST_NEIGHBOR 0
#define FI_GRADIENT_CELL_EDGES 1
#define FI_GRADIENT_LINEAR_INTERPOLATION 2

typedef struct fi_ctx fi_ctx;

/* field_interpolation.hpp:75-95 `Weights`, field for field. */
typedef struct fi_weights {
	float data_pos;
	float data_gradient;
	float model_0, model_1, model_2, model_3, model_4;
	float gradient_smoothness;
	int   value_kernel;
	int   gradient_kernel;
} fi_weights;

/* sparse_linear.hpp:66-73 `SolveOptions`. */
typedef struct fi_solve_options {
	int   tile;
	int   tile_size;
	int   cg;
	int   max_iterations;
	float error_tolerance;
} fi_solve_options;

/* sparse_linear.hpp:8-15 `Triplet` (12 bytes). */
typedef struct fi_triplet {
	int   row, col;
	float value;
} fi_triplet;

/* Counters and timings of the last assemble / solve (the reference logs these through loguru:
 * sparse_linear.cpp:122-125,208-209,438-439). */
typedef struct fi_stats {
	long   num_unknowns;       /* owned lattice points of this rank */
	long   num_data_rows;      /* data rows accepted (value + gradient rows inside the lattice) */
	long   num_cells;          /* distinct lattice cells holding data */
	long   num_generic_rows;   /* rows held in generic (COO) form */
	int    iterations;         /* CG iterations of the last solve */
	int    converged;          /* 1: ||r|| <= tol*||Atb|| reached; 0: stopped by max_iterations.  Under FI_OPT_FIELD_TOLERANCE: 1 when the
	                              field estimate is within the tolerance (or an fp64 recurrence has reached its floor: as converged as
	                              the arithmetic allows); 0 also for an fp32 solve that ends at ITS floor with the estimate above it */
	double rel_residual;       /* recurrence ||r||/||Atb|| at exit */
	double assemble_ms;        /* GPU time of the last fi_assemble */
	double solve_ms;           /* GPU time of the last solve */
	double spmv_ms_avg;        /* mean duration of the AtA-apply launches sampled with HIP events */
	int    spmv_samples;
	double spmv_bytes;         /* algorithmic bytes of one AtA apply */
	int    restarts;           /* residual replacements: b - A x was evaluated this many times at convergence */
	double verified_residual;  /* ||b - A x||/||b|| at the last such evaluation (-1: none) */
	int    num_levels;         /* 1 + coarser levels built by the last fi_assemble */
	int    coarse_iterations;  /* CG iterations spent on coarser levels by the last solve (cascade start); a level solved without
	                              a look at its stop flag (same problem shape and tolerance as the solve before) counts what its
	                              flag said afterwards */
	double prec_ms_avg;        /* mean duration of the sampled Chebyshev-step launches of the polynomial preconditioner */
	int    prec_samples;
	double prec_bytes;         /* mean algorithmic bytes of the sampled launches (every step of the sampled polynomials: 2.5 / 3.5 / 4.5 lattice passes) */
	int    operator_applies;   /* full operator applications + preconditioner steps of the last solve (finest level) */
	int    halo_exchanges;     /* slabs: halo exchanges of the finest level during the last solve (polynomial PCG) */
	int    reductions;         /* slabs: dot-product reductions across the ranks during the last solve (polynomial PCG) */
	int    coarse_unconverged; /* levels of the coarse-to-fine start that had NOT met their tolerance after the iterations their
	                              previous solve had needed (no look at the flag in between): the finest level then started from a
	                              poorer guess and still converged to ITS tolerance; those levels watch their flag again next time */
	double field_estimate;     /* FI_OPT_FIELD_TOLERANCE: estimate of ||x - x*||_inf / ||x||_inf of the returned field at the last
	                              iteration of a solve the rule ran (it may have ended at the floor or max_iterations: see
	                              field_rounds); -1: the residual rule ran -- the option unset, a path without the rule (see
	                              FI_OPT_FIELD_TOLERANCE), or no solve yet */
	double field_per_residual; /* ... change of the field (relative, maximum norm) per unit of relative residual dropped over the
	                              last iteration; 0 when the residual rule ran */
	double stop_residual;      /* the relative residual the last solve ended at (= rel_residual) */
	int    field_rounds;       /* 1: the field test ended the last solve; 0: anything else -- the residual rule, the precision's
	                              floor or max_iterations under FI_OPT_FIELD_TOLERANCE, a path without the rule */
} fi_stats;

const char* fi_last_error(void);
/* Number of visible HIP devices (does not initialise a context). */
int fi_device_count(int* count);

/* ---- context --------------------------------------------------------------------------------
 * Replaces `LatticeField{sizes}` (field_interpolation.hpp:97-111): x (sizes[0]) is the fastest axis.
 * The context lives on the current HIP device. */
int fi_ctx_create(fi_ctx** out, int ndim, const int* sizes, int dtype);

/* Slab-decomposed context for one rank of `nranks` (one process per GPU): the slowest axis
 * (sizes[ndim-1]) is split into contiguous slabs; `sizes` are the GLOBAL lattice sizes.  Every rank
 * passes every data point (or at least those within one cell of its slab); each rank keeps the cells
 * that touch its slab.  Follow with fi_comm_init before fi_assemble. */
int fi_ctx_create_slab(fi_ctx** out, int ndim, const int* sizes, int dtype, int rank, int nranks);
int fi_ctx_destroy(fi_ctx* ctx);

/* Owned range [lo, hi) of the slowest axis for this rank. */
int fi_slab_range(const fi_ctx* ctx, int* lo, int* hi);
/* Data points this rank has to be given: those whose coordinate z along the slowest axis lies in [*lo, *hi).  The
 * range covers every cell that touches the slab on the finest level AND on each of the FI_OPT_LEVELS coarser levels
 * set so far (a coarse cell of level l spans 2^l fine planes, and the coarse replicas are assembled from the rank's
 * own points): call it after fi_set_option(FI_OPT_LEVELS).  Points outside the range are never needed; points inside
 * it that touch no owned plane are dropped by the library. */
int fi_slab_point_range(const fi_ctx* ctx, float* lo, float* hi);
/* The partition rule itself (pure host arithmetic, no GPU): planes [lo, hi) of `planes` for `rank`. */
int fi_slab_partition(int planes, int rank, int nranks, int* lo, int* hi);
/* Ghost planes a slab keeps on each side: the reach of the widest enabled model stencil (model_k -> k),
 * at least 1 (cell blocks and gradient_smoothness reach one plane). */
int fi_halo_width(const fi_weights* w, int* width);

/* Diagnostic: runs the RCCL call pattern of the slab exchange (grouped ncclSend/ncclRecv on a stream, in-place
 * fp64 all-reduce) on a ONE-rank communicator of `device` and checks the data -- the part of the multi-GPU path
 * a single-GPU machine can execute against the real library. */
int fi_comm_self_test(int device, long count);

/* RCCL bootstrap (no reference counterpart: the reference is single-process).  Rank 0 calls
 * fi_comm_unique_id, the 128 bytes are broadcast by the launcher (torch.distributed), every rank calls
 * fi_comm_init.  Halo planes of the CG search direction and the dot products then travel over xGMI. */
int fi_comm_unique_id(void* out128);
int fi_comm_init(fi_ctx* ctx, const void* unique_id128);
/* What the transport of a slab context looks like from the inside (a bench line can then show that RCCL really carried N
 * ranks): out[0] = ranks the communicator counts (ncclCommCount; the test transport: its segment's; 0: no transport),
 * out[1] = this rank's index in it (ncclCommUserRank), out[2] = the HIP device the communicator is bound to
 * (ncclCommCuDevice), out[3] = 1 RCCL / 2 host-staged test transport / 0 none, out[4] = ghost planes one exchange moves
 * to each neighbour (the stencil reach), out[5] = ghost planes stored (the polynomial's deep exchange moves that many
 * once per polynomial), out[6] = bytes of one lattice plane in the context's precision. */
int fi_comm_info(const fi_ctx* ctx, long out[7]);
/* TEST transport for ranks that share one GPU (RCCL refuses two ranks on one device): the halo planes and the dot
 * products travel through the POSIX shared-memory segment `name` ("/...") by host copies, behind the same two internal
 * operations (exchange_halo, allreduce_sum) the RCCL path implements.  Rank 0 passes create = 1 BEFORE the other ranks
 * attach (the launcher orders the calls).  Everything above the wire -- slab geometry, per-rank assembly, the rank-set
 * solvers, bench.py --gpus N -- then runs for real on a single-GPU machine.  Slow by construction; never the product path. */
int fi_comm_init_host(fi_ctx* ctx, const char* name, int create);

/* ---- assembly -------------------------------------------------------------------------------
 * fi_set_model replaces add_field_constraints(field, weights) (field_interpolation.cpp:326-341):
 * the model_0..model_4 and gradient_smoothness rows of add_model_constraint (:243-316) are never
 * materialised; the operator applies them matrix-free.  Only the model_* and gradient_smoothness
 * fields of `w` are read here. */
int fi_set_model(fi_ctx* ctx, const fi_weights* w);

/* Replaces add_points (field_interpolation.cpp:343-371) and, with n == 1, add_value_constraint (:57-80),
 * add_value_constraint_nearest_neighbor (:82-107) and add_gradient_constraint (:123-240).
 *   per point i:  w_i = point_weights ? point_weights[i] : 1
 *     value row    with weight w_i*value_weight  and target values ? values[i] : 0
 *     gradient rows with weight w_i*gradient_weight  when normals != NULL
 * A zero weight skips the rows, points outside the lattice are ignored, exactly as the reference.
 * FI_VALUE_NEAREST_NEIGHBOR requires normals (reference CHECK_NOTNULL_F, :361) -> FI_ERR_INVALID.
 * May be called several times; rows accumulate until fi_assemble. */
int fi_add_points(fi_ctx* ctx, long n, const float* positions, const float* normals, const float* point_weights,
                  const float* values, float value_weight, int value_kernel, float gradient_weight,
                  int gradient_kernel, int memory);

/* The border prior of the reference's SDF application (src/sdf_field.cpp:218-246, generate_sdf_field with
 * boundary_weight > 0): every lattice point on the border of the lattice gets the row [1] * weight = d * weight, d = its
 * distance to the nearest data point given to fi_add_points so far (fp32: sum of squared coordinate differences, min,
 * sqrt -- the reference's arithmetic).  The distance is fi_nearest's (an exact tree search, bit-identical to the reference's
 * O(border x points) loop, which the environment switch FI_BORDER_BRUTE still runs); a slab context: FI_ERR_UNSUPPORTED.  The
 * rows join the data rows (and the coarser levels).  Call it after fi_add_points, before fi_assemble.  weight == 0 adds nothing. */
int fi_add_border_prior(fi_ctx* ctx, float weight);

/* Generic rows: replaces handing an arbitrary `LinearEquation` (sparse_linear.hpp:18-22) to the solvers,
 * as src/bipolar_2d.cpp:177-302 and src/line_2d.cpp:49-104 do.  Duplicate (row, col) entries are summed
 * (sparse_linear.hpp:43) left to right in input order -- the order of the calls, then the order within a call -- in the
 * context's precision (FI_F32: float additions, FI_F64: the float values widened, double additions), as Eigen's
 * setFromTriplets does.  Row indices are local to this call (0..nrows-1).  memory: FI_HOST or FI_DEVICE, for both buffers. */
int fi_add_rows_coo(fi_ctx* ctx, long nrows, long ntriplets, const fi_triplet* triplets, const float* rhs,
                    int memory);

/* Replaces as_sparse_matrix_float + make_square + A^T*b (sparse_linear.cpp:59-70,105-113,120): bins the
 * data rows by lattice cell, accumulates the per-cell A^T A blocks, A^T b and diag(A^T A) on the GPU.
 * Returns when everything is ENQUEUED on the context's stream (sizes the host needs have been read back on the way): the
 * next call on the context -- normally fi_solve_cg -- queues behind it.  fi_stats.assemble_ms is the time between two events
 * around the call's device work; fi_get_stats waits for the second one. */
int fi_assemble(fi_ctx* ctx);

/* Drops all data rows (model weights are kept). */
int fi_clear_points(fi_ctx* ctx);

/* ---- solve ----------------------------------------------------------------------------------
 * Replaces solve_sparse_linear_with_guess (sparse_linear.cpp:186-212) and the CG phase of
 * solve_tiled_with_guess (:427-440).  Jacobi-preconditioned conjugate gradients on A^T A x = A^T b
 * (the reference runs Eigen::BiCGSTAB with the same diagonal preconditioner and the same stop rule
 * ||r||_2 <= tol * ||A^T b||_2).  max_iterations <= 0: 2*N (Eigen default); tol <= 0: fp32 epsilon.
 * guess == NULL means zeros.  `guess`/`out` hold the owned unknowns of this rank (fp32). */
int fi_solve_cg(fi_ctx* ctx, const float* guess, int max_iterations, float tol, float* out, int* iterations,
                float* rel_residual, int memory);

/* Solver options.  FI_OPT_VERIFY_RESIDUAL (default 1): when the recurrence residual meets the tolerance,
 * evaluate b - A x; if it misses the tolerance (fp32 drift) restart CG from it, at most 3 times.  0 gives
 * the reference's stop rule on the recurrence residual alone.
 * FI_OPT_LEVELS (default 0): coarser replicas of the problem (lattice halved per level, weights rescaled,
 * the same data points) built by fi_assemble; with guess == NULL, fi_solve_cg then starts from a coarse-to-fine
 * cascade (each level solved to FI_OPT_COARSE_TOLERANCE, default 1e-3, and interpolated to the next) -- the
 * reference's recipe for large lattices (src/sdf_field.cpp:272-288, README.md "My resolution is huge"),
 * generalised to several levels and kept on the device. */
#define FI_OPT_VERIFY_RESIDUAL 1
#define FI_OPT_LEVELS 2
#define FI_OPT_COARSE_TOLERANCE 3
/* FI_OPT_MULTIGRID (default 0): with levels, precondition CG with one V-cycle over them (Chebyshev-Jacobi
 * smoothing, R = P^T, coarse operators re-assembled from the same points) instead of the Jacobi diagonal. */
#define FI_OPT_MULTIGRID 4
/* FI_OPT_MIXED_PRECISION (default 0; FI_F64 contexts, with FI_OPT_LEVELS and FI_OPT_MULTIGRID): fi_assemble also
 * builds an fp32 replica of the problem and gives IT the levels; CG (x, r, p, the operator apply, every dot
 * product and the stop test) stays in fp64, the V-cycle preconditioner -- most of the HBM traffic of an iteration
 * -- runs on the replica in fp32 (z = s V32(r / s), s = ||r||/||b||).  Same iteration counts and answers as the
 * pure fp64 solve, about 0.7x the time.  The SDF configurations need fp64 residuals: in fp32 alone b - A x stalls
 * near 1e-4 (kappa ~ side^4).  With guess == NULL the coarse-to-fine start also runs on the replica. */
#define FI_OPT_MIXED_PRECISION 5
/* FI_OPT_POLY_TERMS (default 0 = the Jacobi diagonal, Eigen's DiagonalPreconditioner as in sparse_linear.cpp:199): with
 * d >= 2, CG is preconditioned by a Chebyshev polynomial of d terms in Dinv (A_model + diag(A_data)) over the interval
 * [hi / FI_OPT_POLY_RATIO, hi] (default ratio 10; hi = 1.1 x the largest eigenvalue of the Jacobi-scaled model operator,
 * found once per model by the power method).  Same stop rule, same answers; about the same number of operator
 * applications as Jacobi-PCG but d - 1 of every d run as ONE 5-pass launch without cell records, and dot products
 * are reduced twice per d applications.  3-D lattices with model_0 / model_1 / model_2; other contexts ignore it. */
#define FI_OPT_POLY_TERMS 6
#define FI_OPT_POLY_RATIO 7
/* FI_OPT_MG_SMOOTHER (default 1): the V-cycle's smoother on fp32 3-D levels with model_0 / model_1 / model_2.
 * 1: the polynomial of FI_OPT_POLY_TERMS' kind in A_model + f diag(A_data) -- plain-stencil launches without cell
 * records, two full applies per level and cycle; f = FI_OPT_MG_SAFE_FACTOR (default 4; 2^D makes that operator a bound of
 * the full one, so the smoother converges for any data).  0: the Chebyshev polynomial in the full operator on every
 * level (the only smoother of 2-D / fp64 levels).  Both give symmetric positive definite preconditioners. */
#define FI_OPT_MG_SMOOTHER 8
#define FI_OPT_MG_SAFE_FACTOR 9
/* FI_OPT_MG_TERMS (default 5, 2..16) and FI_OPT_MG_RATIO (default 30, (1, 1000]): the polynomial smoother's number of
 * terms (terms - 1 launches of the plain marching kernel per smoothing pass) and the ratio of its interval [hi / ratio, hi].
 * Measured on config 4 (fp64 CG + fp32 V-cycle to a field within 1e-5; profiles/r4_ablation.md): 4 terms / ratio 10 (the
 * setting of round 3) 7 iterations at 256^3 and 8 at 512^3, 5 / 30 five and six -- each cycle 8 % dearer, the solve 20 %
 * cheaper. */
#define FI_OPT_MG_TERMS 10
#define FI_OPT_MG_RATIO 11
/* FI_OPT_FIELD_TOLERANCE (default 0 = off; V-cycle PCG; over slabs up to 16 of them -- their maxima travel with the r . r
 * sum of the iteration's all-reduce, every rank decides on the same numbers): stop by the FIELD, not by the residual --
 * the north-star's accuracy "values within 1e-5 of the CPU reference's double solve" (sparse_linear.cpp:154-184) is a statement
 * about x, and what a residual buys in x varies with the lattice, the data and the weights by three orders of magnitude
 * (kappa ~ side^4).  x* - x_k is the sum of the steps still to come; every iteration the solver holds the last step's size,
 * ||x_k - x_(k-1)||_inf = |alpha| ||p||_inf (a by-product of the pass that updates x), and the history of the residual norms.
 * If the steps shrink by sigma per iteration, ||e_k||_inf <= ||x_k - x_(k-1)||_inf sigma / (1 - sigma).  sigma is the SLOWEST
 * mean decay of the residual norm over the last 1, 2, 4, 8, 16 iterations and over the whole solve, the step the largest of
 * the last nine carried forward at that rate (a slowly converging solve has lucky single drops; its late, faster phases
 * are not the tail's rate; and CG on an ill-conditioned system converges in stairs -- a lull of several iterations with tiny
 * steps and a falling residual while the error stands still, then the next stair); where every one of those windows gains
 * more than a factor 3 per iteration -- a healthy V-cycle -- the last step and its own ratio ||r_k|| / ||r_(k-1)|| are used.
 * The solve ends when twice that (a margin for the smooth modes, which converge last) is within the tolerance times
 * ||x_k||_inf; no estimate is formed while the residual falls by less than 5 % per iteration (the residual floor then ends
 * the solve) and no stop before the third iteration (CG's first steps remove the rough part of the error: small steps, a
 * falling residual, the smooth part not yet moved) -- the eighth behind a caller's guess, whose error may be smooth from the start.  The `tol` of fi_solve_cg is ignored (the precision's floor stands in:
 * 1e-13 in fp64, 2e-7 in fp32 -- an fp32 solve that ends there with the estimate above the tolerance reports converged = 0);
 * no constant depends on the workload.  An estimate, not a bound: over 200 random 3-D, 150 random 2-D and 100 random fp32
 * problems (tests/stress_field_rule.py: value data and oriented points, 1 to 5 levels, 6 to 650 iterations) the true error
 * exceeded the tolerance in 3, 7 and 0 cases (warm starts included; 3 and 9 of 150 + 150 with FI_OPT_MG_KCYCLE), by at most 1.5 x and 2.4 x --
 * but for warm starts on hierarchies whose cold solves take a thousand iterations (2 cases, 15 x); the goldens of configs 2 to 5 end 8 to 100 x
 * below it.  fi_stats: field_estimate, field_per_residual, field_rounds.
 * Paths without the rule stop by the residual at the `tol` of fi_solve_cg, as with the option unset, and report
 * field_estimate = -1, field_per_residual = 0, field_rounds = 0: FI_OPT_MULTIGRID off (Jacobi or polynomial PCG), no coarser
 * level built (a lattice too small to halve, rows from fi_add_rows_coo), more than 16 slabs, and a finest level held as
 * replicated copies. */
#define FI_OPT_FIELD_TOLERANCE 12
/* FI_OPT_MG_KCYCLE (default 0 = off; V-cycle PCG, fp32 levels): a K-cycle -- the correction of the
 * first `value` coarse levels is not one application of the coarser level's cycle but TWO steps of flexible CG on that
 * level's system, each preconditioned by the level's cycle (Notay & Vassilevski: the lengths of the two corrections come from
 * a line search in the energy norm, so a level whose own cycle overcorrects -- the re-discretised coarse levels of
 * oriented-point data do, profiles/r6_ablation.md section 11 -- cannot make the preconditioner indefinite the way a W-cycle
 * does).  Levels the small-level engine runs (<= 4 096 unknowns at the bottom of the hierarchy) keep their V-cycle.  The
 * preconditioner then depends on its argument: the outer CG takes the flexible beta, -alpha z_(k+1) . A p_k / (z_k . r_k),
 * one more dot product per iteration.
 * Over slabs (a loop-back group, or one slab per process) the same algorithm: the same K-levels -- chosen on the undivided
 * lattice, alike on every rank -- and the same steps; only the order of the sums and the collectives differ.  A visit of a
 * slab K-level costs TWO all-reduces (the two dot products of step 1, the four of step 2, each set in one); a K-level's
 * coarser levels are visited twice as often, so the K-levels below the first cost 2, 4, ... per outer iteration, and a
 * junction sum above the replicated tail is made once per visit of its level.  Replicated levels (whole lattices below the
 * slabs) correct on every rank on their own: no collective.  The outer CG's extra dot product travels in the r . z sum: no
 * collective of its own.  fi_stats.reductions counts them all.  Set before fi_assemble. */
#define FI_OPT_MG_KCYCLE 13
/* FI_OPT_MG_CHEB_DEGREE (0 or 2..16) and FI_OPT_MG_CHEB_RATIO (0 or (1, 1000]): degree and interval [lambda / ratio, 1.1 lambda] of
 * the Chebyshev smoother in the full operator (2-D lattices, oriented points, fp64 levels).  0 (default): by the lattice's
 * dimension -- 4 over [lambda / 10] in 2-D, 5 over [lambda / 40] in 3-D (swept under the field rule with the V-cycle).  With
 * the K-cycle on a deep hierarchy the coarse correction is strong and the smoother need not reach down: config 5 runs (4, 10)
 * (profiles/r6_ablation.md section 12).  Set before fi_assemble. */
#define FI_OPT_MG_CHEB_DEGREE 14
#define FI_OPT_MG_CHEB_RATIO 15
int fi_set_option(fi_ctx* ctx, int option, double value);

/* Replaces jacobi_iterations (sparse_linear.cpp:214-241): x <- x + w*(Atb - AtA x)/diag, true Jacobi. */
int fi_jacobi(fi_ctx* ctx, const float* guess, int num_iterations, float weight, float* out, int memory);

/* Replaces tile_solver_square (sparse_linear.cpp:246-390), the pre-solver behind SolveOptions.tile
 * (solve_tiled_with_guess :415-425): non-overlapping tile_size^D tiles, every tile solved for its own unknowns
 * with the couplings to other tiles moved to the right-hand side using `guess` (the reference moves every
 * off-tile coupling twice, :327-334 -- reproduced), 1e-6 added to the tile diagonals (:296-300).  The tiles are
 * independent SPD systems; they are solved together by one CG run on the block-diagonal tile operator
 * (fp32 contexts to a relative residual of 1e-6, fp64 to 1e-12) instead of one sparse Cholesky per tile.
 * Lattice rows (fi_set_model / fi_add_points) and fi_add_rows_coo rows alike -- the rows of a materialised
 * LinearEquation are split into their per-tile pieces on the fly; in a context of such rows only, a tile without
 * any entry keeps the guess, as the reference skips it.  tile_size >= 2 (:254). */
int fi_tile_pass(fi_ctx* ctx, const float* guess, int tile_size, float* out, int memory);

/* Replaces generate_error_map (field_interpolation.cpp:402-429): the blame heat-map of a solution.  Every
 * equation (model row, data row, fi_add_rows_coo row) distributes its squared residual (rhs - a.x)^2 over its
 * unknowns in proportion to a_j^2.  `solution` and `out`: owned unknowns, x fastest, fp32.  Rows added by
 * fi_add_points are read from the row tables of the last batches (kept until fi_clear_points). */
int fi_error_map(fi_ctx* ctx, const float* solution, float* out, int memory);

/* ---- robust fits: data points reweighted by their residuals ------------------------------------
 * Iteratively reweighted least squares for data with gross errors: solve, measure every point's residual, lower the weight
 * of the points that disagree with the fit, solve again from the previous field.  The contract ("Robust
 * fits") is this project's own; the reference has no counterpart (its demo only injects the outliers, src/sdf_field.cpp:323-328).
 *   - a DATA POINT is a point of a fi_add_points batch that is not a border-prior batch; points are numbered in call order,
 *     then by order within a call; a context of n points uses these numbers in every buffer below;
 *   - residual of a point: its rows as fi_add_points forms them with the point weight set to 1 (cw = value_weight for the value
 *     row, gradient_weight for the gradient rows).  Per row e = sum_q c[q] x[corner q] - b, q = 0 .. 2^D - 1 left to right
 *     (corners outside the lattice have c = 0 and are not read); r = sqrt(e_value^2 + e_0^2 + ... + e_(D-1)^2), squared and
 *     added in that order over the rows the point emits.  FI_F32 contexts: every operation in float.  FI_F64 contexts:
 *     coefficients and rhs formed in float exactly as the rows are, then widened; x, the sums and the sqrt in double; r rounded
 *     to float once.  A point that emits no row (outside the lattice, non-finite, base weight 0) has r = -1 and takes no part
 *     in anything below;
 *   - scale: M = the points with r >= 0, med = the element of rank (M - 1) / 2 (integer division) of their r in ascending
 *     order, s = 1.4826f * med in float; a caller's scale > 0 replaces it;
 *   - weight factor, all in float: u = r / (s * c), the product formed first; c the tuning constant, 0 = the loss's default:
 *       FI_LOSS_HUBER   c = 1.345   omega = u <= 1 ? 1 : 1 / u
 *       FI_LOSS_CAUCHY  c = 2.385   omega = 1 / (1 + u * u)
 *       FI_LOSS_TUKEY   c = 4.685   omega = u < 1 ? (1 - u * u)^2 : 0, the square as one product
 *     points with r = -1 keep omega = 1;
 *   - new point weight pw_i = base_i * sqrtf(omega_i): a row weight enters the objective squared, so this puts omega on the
 *     point's squared residual.  base_i is the weight the caller gave, or 1; it is kept and never overwritten: every
 *     reweighting starts from base, not from the last omega;
 *   - s = 0 (more than half of the points fit exactly): the step changes nothing and reports scale 0; a loop ends there.
 * FI_ERR_UNSUPPORTED: slab contexts and group members (a rank holds only its own points and the median is global, as for
 * fi_add_border_prior); contexts that hold fi_add_rows_coo rows; batches with FI_GRADIENT_LINEAR_INTERPOLATION, whose rows
 * live among the generic rows.  FI_ERR_STATE: no data points; no field given and no last solution.  Border-prior batches are
 * re-emitted unchanged.  Residuals measure disagreement with the FIT: an outlier the field can bend to (an oriented point in
 * empty space under a weak model) keeps a small residual and its weight -- the leverage-point limit, DESIGN.md 4.10. */
#define FI_LOSS_HUBER 0
#define FI_LOSS_CAUCHY 1
#define FI_LOSS_TUKEY 2

typedef struct fi_robust_options {
	int   loss;             /* FI_LOSS_* */
	float tuning;           /* c; 0: the loss's default */
	float scale;            /* s; 0: 1.4826 x the median residual */
	int   rounds;           /* fi_solve_robust: reweighted solves at most */
	float weight_tolerance; /* fi_solve_robust: end when max_i |omega_new - omega_old| is below it; 0: never */
} fi_robust_options;

typedef struct fi_robust_stats {
	int    rounds;            /* reweighted solves done (the first, plain solve is not counted) */
	int    iterations;        /* CG iterations of all solves */
	float  scale;             /* s of the last reweighting step */
	float  max_weight_change; /* max_i |omega_new - omega_old| of the last reweighting step */
	long   points_used;       /* M of the last reweighting step */
	long   points_zeroed;     /* points with r >= 0 whose omega is 0 after it */
	double reweight_ms;       /* host time of all reweighting steps (residuals, scale, weights, rows re-emitted) */
} fi_robust_stats;

/* the number of data points of the context */
int fi_point_count(const fi_ctx* ctx, long* n);
/* residuals: float[n].  field: the context's owned values (fp32), or NULL for its last solution where it lives (FI_F64: in
 * full precision).  `memory` applies to field and residuals. */
int fi_point_residuals(fi_ctx* ctx, const float* field, float* residuals, int memory);
/* One step: residuals -> scale -> omega -> point weights; the rows are emitted again from the points, in the order of the
 * first emission, so the context then holds the rows a fresh one holds that was given base * sqrt(omega) as point weights.
 * Only loss, tuning and scale of the options are read.  omega: float[n] or NULL; scale: the s used, or NULL.  The context
 * needs fi_assemble afterwards (not when the step reports scale 0). */
int fi_robust_reweight(fi_ctx* ctx, const float* field, const fi_robust_options* options, float* omega, float* scale, int memory);
/* back to the caller's weights (every omega 1); needs fi_assemble */
int fi_reset_point_weights(fi_ctx* ctx);
/* Assembles if needed; solves from `guess` (NULL: zeros, or the coarse-to-fine start where levels are set); then up to
 * options->rounds times: reweights from the current field, assembles, solves from the current field.  Ends early at scale 0
 * and, after the solve, when the step's max |omega_new - omega_old| < weight_tolerance.  Every solve is fi_solve_cg with
 * max_iterations and tol, under whatever solver options the context carries (levels, V-cycle or K-cycle, mixed precision,
 * field tolerance); the coarser levels and the fp32 replica pick the weights up through the re-assembly.  Afterwards the
 * context holds the last weights: fi_error_map, fi_true_residual and a later fi_solve_cg see the robust system.
 * out: the owned unknowns (fp32); omega: float[n] or NULL; stats may be NULL.  `memory` applies to guess, out and omega. */
int fi_solve_robust(fi_ctx* ctx, const float* guess, const fi_robust_options* options, int max_iterations, float tol, float* out,
                    float* omega, fi_robust_stats* stats, int memory);

/* fp64 copy of the last solution (FI_F64 contexts keep full precision; FI_F32 widens). Host buffer. */
int fi_get_solution_f64(fi_ctx* ctx, double* out);

/* True residual ||Atb - AtA x||_2 / ||Atb||_2 of the last solution, evaluated on the GPU. */
int fi_true_residual(fi_ctx* ctx, double* rel_residual);

/* ---- test / measurement hooks (host buffers, owned unknowns) ------------------------------------ */
int fi_apply_AtA_f64(fi_ctx* ctx, const double* x, double* y); /* y = (A^T A) x */
int fi_get_Atb_f64(fi_ctx* ctx, double* out);
int fi_get_diag_f64(fi_ctx* ctx, double* out);
int fi_get_stats(const fi_ctx* ctx, fi_stats* out);
/* Device memory of destroyed contexts is kept (per device, at most 8 GiB) and handed to the next context: hipMalloc /
 * hipFree synchronise the device and dominate the cost of a context that lives for one solve -- what a caller of the
 * reference's stateless solve_sparse_linear* (sparse_linear.hpp:75-96) creates per call.  Frees pooled blocks of the
 * CURRENT device down to keep_bytes (0: everything; negative: nothing) and reports what stays cached. */
int fi_memory_pool(long long keep_bytes, long long* cached_bytes);
/* Launches the AtA apply `reps` times on the context's stream between two HIP events. */
int fi_time_apply(fi_ctx* ctx, int reps, double* ms_per_launch);

/* ---- loop-back group (test facility) ---------------------------------------------------------------
 * All `nranks` slabs of a decomposition in ONE process on the current device: the same kernels, slab
 * geometry, halo widths and ownership rules as the RCCL path, with halo planes moved by device-to-device
 * copies and dot products summed by a kernel.  Lets a single GPU check the decomposed solve against the
 * undivided one.  Per-rank assembly goes through fi_group_rank(g, r) and the fi_set_model / fi_add_points
 * calls above; vectors passed to the group calls are host buffers holding the WHOLE lattice. */
typedef struct fi_group fi_group;
typedef struct fi_mesh fi_mesh;
typedef struct fi_points fi_points;
typedef struct fi_surface fi_surface;
int     fi_group_create(fi_group** out, int ndim, const int* sizes, int dtype, int nranks);
int     fi_group_destroy(fi_group* g);
int     fi_group_size(const fi_group* g);
fi_ctx* fi_group_rank(fi_group* g, int rank);
int     fi_group_assemble(fi_group* g);
int     fi_group_solve_cg(fi_group* g, const float* guess, int max_iterations, float tol, float* out, int* iterations,
                          float* rel_residual);
int     fi_group_apply_AtA_f64(fi_group* g, const double* x, double* y);
int     fi_group_true_residual(fi_group* g, double* rel_residual);
int     fi_group_get_solution_f64(fi_group* g, double* out);
int     fi_group_tile_pass(fi_group* g, const float* guess, int tile_size, float* out);
int     fi_group_error_map(fi_group* g, const float* solution, float* out);
/* iso-contours of the group's field (see fi_iso_extract below): whole_or_null is the WHOLE lattice on the host, or NULL for
 * the members' last solution; out receives nranks meshes, piece r holding the cells of slab r (see fi_iso_extract). */
int     fi_group_iso_extract(fi_group* g, const float* whole_or_null, float iso, fi_mesh** out);
/* point queries of the group's field (see fi_sample below): whole_or_null is the WHOLE lattice, or NULL for the members' last
 * solution; positions, values and gradients are host buffers, the results are those of the undivided lattice */
int     fi_group_sample(fi_group* g, const float* whole_or_null, long n, const float* positions, int mode, float fill,
                        float* values, float* gradients);

/* ---- helpers either side of the path ---------------------------------------------------------
 * Replaces upscale_field (field_interpolation.cpp:431-485): multilinear resampling small -> large. */
int fi_upscale_field(const float* small_field, int ndim, const int* small_sizes, const int* large_sizes,
                     float* out, int memory);

/* ---- iso-contours and iso-surfaces -----------------------------------------------------------
 * After the solve, what src/sdf_field.cpp:605-613 (iso_surface) does on the host: the lattice's iso-contour, extracted on the
 * device.  2-D: marching squares, line segments; 3-D: marching cubes, triangles; 1-D: FI_ERR_UNSUPPORTED.  The contract
 * ("Iso-contours and iso-surfaces") is this project's own:
 *   - inside is f < iso; one vertex per lattice edge (p, p + e_a) whose ends differ in inside-ness, at coordinate
 *     p_a + t along a, t = dp / (dp - dq), dp = f(p) - iso, dq = f(q) - iso in fp32; key ndim * index(p) + a, vertices in
 *     ascending key order; positions in lattice units;
 *   - normal: (1 - t) g(p) + t g(q) normalised, g = central differences (one-sided at the border), towards increasing f;
 *   - cells (all corners in the lattice) in ascending linear index; a face with two diagonal inside corners cuts each off
 *     by its own segment (the 3-D mesh is watertight); 2-D segments have the inside on their left, 3-D triangles
 *     (a, b, c) have (b - a) x (c - a) pointing from inside to outside;
 *   - a non-finite value: FI_ERR_INVALID and no mesh; a mesh of >= 2^31 vertices: FI_ERR_UNSUPPORTED (int32 indices).
 * The mesh stays on the device until fi_mesh_copy; the caller destroys it with fi_mesh_destroy.
 *
 * field: the context's owned values (host or device per `memory`); NULL = the context's last solution, read where it lives
 * (an FI_F64 solution is rounded to fp32 first, exactly as fi_solve_cg's `out` is).  A slab context (nranks > 1, with its
 * transport) exchanges the ghost planes it needs and returns its piece: the cells whose slowest coordinate lies in its
 * slab, with every vertex they use (seam vertices too, under their global keys).  Pieces concatenated in rank order and
 * de-duplicated by key give the undivided mesh. */
int fi_iso_extract(fi_ctx* ctx, const float* field, float iso, int memory, fi_mesh** out);
/* the same without a context: any whole field (e.g. the output of fi_upscale_field) */
int fi_iso_extract_field(const float* field, int ndim, const int* sizes, float iso, int memory, fi_mesh** out);

/* ---- dual contouring ------------------------------------------------------------------------
 * The same kind of mesh, but with one vertex per crossed cell, placed by the least-squares fit of the reference's
 * src/dual_contouring_2d.cpp (which its app never calls), so that sharp corners and edges survive.  The contract (DESIGN.md
 * 4.8, "Dual contouring") -- everything is computed from d = f - iso in fp32, one rounding per operation:
 *   - inside is d <= 0 (the reference's rule; fi_iso_extract's is f < iso).  A non-finite d: FI_ERR_INVALID; a 1-D lattice:
 *     FI_ERR_UNSUPPORTED; an extent < 2: an empty mesh and FI_OK;
 *   - gradients: ndim floats per lattice point, interleaved, x fastest (the reference's Vec2*), used as given; NULL: the
 *     reference's calculate_gradients per axis, (d[+1] - d[-1]) / 2, one-sided at that axis's own border (the reference tests
 *     y == width - 1 for the y border and so reads out of bounds on non-square lattices; parity with it is claimed on square
 *     lattices, or with gradients passed in);
 *   - cells (all corners in the lattice) in ascending linear index, x fastest; corner i steps +1 along axis k where bit k of i
 *     is set.  A cell has a vertex unless its corners are all inside or all outside; crossing[i]: some cell edge at corner i
 *     joins corners of different inside-ness;
 *   - the fit: 2^D + D rows.  Corner rows first, in corner order: A_i = g(corner_i), b_i = ((bit_0 g_0 + bit_1 g_1)
 *     [+ bit_2 g_2]) - d_i, a zero row where crossing[i] is not set; then D rows r e_k with right-hand side 0.5f r.  A^T A and
 *     A^T b accumulate over the rows in order.  2-D: solve_lin_eq_2d, det = M0 M3 - M1 M2, x = (b0 M3 - M1 b1) / det,
 *     y = (b1 M0 - M2 b0) / det.  3-D: Cramer's rule, x_k = det3(M with column k replaced by A^T b) / det3(M), with
 *     det3(a) = (a0 c0 - a1 c1) + a2 c2, c0 = a4 a8 - a5 a7, c1 = a3 a8 - a5 a6, c2 = a3 a7 - a4 a6 (row-major).  r starts at
 *     0.001f and doubles while any coordinate is < 0 or > 1 (a NaN ends the loop, as the reference's do ... while), for at most
 *     32 solves; a vertex that is then non-finite or outside [0, 1]^D is the cell centre.  Position (float)cell_k + v_k, key
 *     the lattice index of the cell's lowest corner (ascending);
 *   - normal: the corner gradients weighted as fi_sample's FI_SAMPLE_LINEAR weighs corner values at the offset v, summed in
 *     ascending corner order, then normalised (a zero gradient stays zero); it points towards increasing f;
 *   - primitives: the lattice edge (p, p + e_a) gives one when its ends differ in inside-ness and every cell around it exists
 *     (2 in 2-D, 4 in 3-D).  Its lowest cell p - sum_(k != a) e_k emits it; cells emit in ascending index, within a cell by
 *     axis a from D - 1 down to 0.  2-D: the reference's order and orientation (the inside on the left): a = 1, the +x
 *     neighbour, (this, it) when p + e_a is inside, else (it, this); a = 0, the +y neighbour, (it, this) when p + e_a is inside,
 *     else (this, it).  3-D: the cells q0 .. q3 at offsets (0,0), (1,0), (1,1), (0,1) along b = (a+1)%3, c = (a+2)%3 from the
 *     lowest form a quad with normal +a, reversed to (q0, q3, q2, q1) when p is outside; triangles (q0, q1, q2), (q0, q2, q3)
 *     of the quad so ordered, so that (b - a) x (c - a) points from inside to outside;
 *   - int32 indices (>= 2^31 vertices: FI_ERR_UNSUPPORTED); no atomics in the outputs: the bytes do not depend on the run or
 *     the launch shape.
 * field NULL: the context's last solution where it lives (an FI_F64 solution is rounded to fp32 once, as fi_iso_extract
 * does); `memory` applies to field and gradients.  Slab contexts (nranks > 1): FI_ERR_UNSUPPORTED -- the vertices of a slab's
 * first cell plane above it need field planes hi .. hi + 2 (the last for the central differences), one more than the two
 * ghost planes of the iso path, so slabs need a vertex exchange; there is no group entry either. */
int fi_dual_contour(fi_ctx* ctx, const float* field, const float* gradients, float iso, int memory, fi_mesh** out);
/* the same without a context: any whole field, fp32, x fastest */
int fi_dual_contour_field(const float* field, const float* gradients, int ndim, const int* sizes, float iso, int memory,
                          fi_mesh** out);

int fi_mesh_info(const fi_mesh* m, long* num_vertices, long* num_primitives, int* vertices_per_primitive);
/* any output may be NULL; vertices / normals are ndim floats per vertex, indices vertices_per_primitive int32 per primitive */
int fi_mesh_copy(const fi_mesh* m, float* vertices, float* normals, int* indices, long long* keys, int memory);
int fi_mesh_destroy(fi_mesh* m);

/* ---- the connected parts of a mesh ------------------------------------------------------------
 * Labels a device mesh's connected parts, says what each part is, and keeps a chosen subset, without the mesh leaving the
 * device.  Works on the meshes of fi_iso_extract* / fi_dual_contour* (a slab piece's parts are the piece's own) and on meshes
 * the caller brings (fi_mesh_create).  The contract (tests/mesh_parts_reference.py is its definition in numpy):
 *   - parts: two primitives belong to one part when a chain of primitives joins them, each sharing a vertex INDEX with the
 *     next (coincident positions under different indices do not join).  A vertex no primitive uses has label -1 and belongs
 *     to no part.  Parts are numbered 0 .. C-1 by their smallest vertex index, ascending; labels are int32 and do not depend
 *     on the run or the launch shape.  An empty mesh: 0 parts, FI_OK.  The labelling is computed at the first of the three
 *     calls below that needs it and kept with the handle (meshes are immutable);
 *   - counts, exact.  A half-edge is a directed index pair of a primitive: (a,b), (b,c), (c,a) of a triangle, (a,b) of a
 *     segment; half-edges with equal ends are ignored.  `vertices` and `primitives` count the part's used vertices and its
 *     primitives.  3-D: `edges` the distinct unordered pairs, `boundary` the pairs used by exactly one half-edge, `irregular`
 *     the pairs used by more than two half-edges or by two of the same direction.  2-D: `edges` the half-edges, `boundary`
 *     the vertices of total degree 1, `irregular` the used vertices that have neither degree 1 nor (in, out) = (1, 1).
 *     A part is CLOSED when boundary == 0 && irregular == 0; its Euler characteristic in 3-D is vertices - edges + primitives;
 *   - measures, fp64 from the fp32 coordinates converted exactly, one rounding per operation.  3-D: size = sum of
 *     |(b-a) x (c-a)| / 2 (the area), enclosed = sum of a . (b x c) / 6.  2-D: size = sum of |b-a| (the length), enclosed =
 *     sum of (a_x b_y - a_y b_x) / 2.  With the extractors' orientation `enclosed` is positive for a blob of inside and
 *     negative for a cavity; it means something only for a closed part (the sum over an open part depends on the origin).
 *     The sums are taken in a fixed order (chunks of 256 of the part's primitives in ascending primitive number, each summed
 *     by a fixed tree, the chunks added in ascending order) without floating-point atomics: a repeated call returns the same
 *     bytes.  lo / hi: the per-axis fp32 extremes of the part's vertices (2-D: lo[2] = hi[2] = 0);
 * fi_mesh_create: vertices ndim floats per vertex, indices ndim int32 per primitive, all in `memory`.  ndim other than 2 or 3:
 * FI_ERR_UNSUPPORTED (as fi_surface_create); an index outside [0, num_vertices): FI_ERR_INVALID and no mesh; a count >= 2^31:
 * FI_ERR_UNSUPPORTED; a negative count or a null array of a non-zero count: FI_ERR_INVALID.  keys NULL: the keys 0 .. V-1.
 * normals NULL: the mesh has no normals -- fi_mesh_copy of it (and of whatever fi_mesh_select makes of it) refuses a normals
 * buffer with FI_ERR_INVALID.
 * fi_mesh_parts: the labels into arrays in `memory` (num_vertices / num_primitives int32; either may be NULL).
 * fi_mesh_measure: parts is a HOST array of `capacity` rows; *num_parts is always set; capacity < *num_parts: FI_ERR_INVALID
 * and nothing written (parts may be NULL with capacity 0 to ask for the count).
 * fi_mesh_select: keep is a HOST array, one byte per part (non-zero: kept); num_parts must equal the mesh's count, else
 * FI_ERR_INVALID.  The result holds the vertices of the kept parts in their original order with their normals and keys (the
 * keys stay ascending; unused vertices are dropped) and the kept primitives in their original order with their indices
 * remapped.  No atomics write an output.  Keeping everything on a mesh without unused vertices returns the same arrays;
 * keeping nothing an empty mesh. */
typedef struct fi_mesh_part {
	long long vertices, primitives, edges, boundary, irregular;
	double    size, enclosed;
	float     lo[3], hi[3];
} fi_mesh_part;
int fi_mesh_create(fi_mesh** out, int ndim, long num_vertices, const float* vertices, const float* normals,
                   const long long* keys, long num_primitives, const int* indices, int memory);
int fi_mesh_parts(const fi_mesh* m, long* num_parts, int* vertex_labels, int* primitive_labels, int memory);
int fi_mesh_measure(const fi_mesh* m, long capacity, fi_mesh_part* parts, long* num_parts);
int fi_mesh_select(const fi_mesh* m, long num_parts, const unsigned char* keep, fi_mesh** out);

/* ---- mesh simplification: vertex clustering with quadric placement ------------------------------
 * Makes a device mesh coarser -- or, with a cell below the vertex spacing, welds the coincident vertices of a triangle soup
 * -- without the mesh leaving the device: the vertices of one cube of a uniform grid become one vertex (Rossignac-Borrel),
 * placed at the minimum of the cluster's quadric error function (Lindstrom 2000) or at the cluster's mean.  Any fi_mesh, 2-D
 * segments or 3-D triangles, with or without normals.  The contract (tests/simplify_reference.py is its
 * definition in numpy):
 *   - cells: only USED vertices take part (those some primitive references).  c_a = floorf((p_a - o_a) / cell) in fp32, one
 *     rounding per operation; origin: ndim floats on the HOST, NULL = 0.  A non-finite coordinate of a used vertex, or
 *     |c_a| >= 2^20: FI_ERR_INVALID and no mesh.  The cell key is sum_a (c_a + 2^20) << 21 a (int64); the clusters are the
 *     distinct keys, ascending; the cell centre g = o + (c + 1/2) cell in fp64;
 *   - primitives: indices replaced by cluster numbers; a primitive with two equal indices is dropped; of the primitives with
 *     the same ORIENTED tuple (3-D: the triple rotated so that its smallest index comes first; 2-D: the ordered pair) only
 *     the lowest-numbered stays -- a primitive and its reverse are different tuples and both stay.  Survivors keep their
 *     input order and winding;
 *   - output vertices: the clusters a surviving primitive references, in ascending key order; their keys are the output
 *     mesh's keys (ascending).  vertex_map (optional, int32 per input vertex, in `memory`): the output vertex of every input
 *     vertex; -1 for an unused vertex and for a cluster that did not survive;
 *   - placement: fp64 from the fp32 coordinates, relative to g (p' = p - g), one rounding per operation, every sum serial in
 *     ascending order from 0.  mean = (sum of the cluster's used vertices in ascending vertex number) / their number.
 *     FI_SIMPLIFY_MEAN: x' = mean.  FI_SIMPLIFY_QUADRIC: every input primitive adds to each DISTINCT cluster among its
 *     vertices, in ascending primitive number, A += n n^T and b += n (n . a'), with n = (b' - a') x (c' - a') in 3-D
 *     (n_x = u_y w_z - u_z w_y, ...; n . a' = (n_x a'_x + n_y a'_y) + n_z a'_z) and n = (-e_y, e_x), e = b' - a', in 2-D, not
 *     normalised (squared-area weights; zero-area primitives add zeros).  r = b - A mean, row i as b_i - ((A_i0 mean_0 +
 *     A_i1 mean_1) + A_i2 mean_2).  The eigenpairs (lambda_i, v_i) of A come from the cyclic Jacobi iteration of
 *     fi_estimate_normals (6 sweeps over the pairs (0,1), (0,2), (1,2), no early exit; v_i the columns); x' = mean, then for
 *     i = 0, 1, 2 with lambda_max > 0 and lambda_i > 1e-3 lambda_max: x' += v_i ((v_i . r) / lambda_i).  A non-finite x', or
 *     any |x'_a| > cell, falls back to the mean: a vertex may leave its cell by half a cell, not more.
 *     Position = (float)(g + x');
 *   - normals, if the mesh has them: the fp64 sum of the members' normals in ascending vertex number, divided by its length
 *     (sqrt of the squares summed in axis order), cast to fp32; a zero sum gives zeros.  A mesh without normals gives a mesh
 *     without normals (fi_mesh_copy of it refuses a normals buffer);
 *   - an empty mesh, or one whose primitives all collapse: an empty mesh and FI_OK (vertex_map all -1).  cell NaN or <= 0, a
 *     bad placement, a bad memory kind, a NULL mesh or out: FI_ERR_INVALID.
 * No floating-point atomics and no atomics in the outputs: a repeated call returns the same bytes.  A cell that swallows most
 * of a mesh makes one thread sum most of it: correct, and slow.  Not offered: a target count (bisect on cell), edge-collapse
 * decimation, boundary or topology preservation (clustering may pinch a thin sheet: fi_mesh_measure of the result reports
 * it as irregular edges), slab groups (merge the pieces first), 1-D. */
#define FI_SIMPLIFY_QUADRIC 0
#define FI_SIMPLIFY_MEAN    1
int fi_mesh_simplify(const fi_mesh* m, float cell, const float* origin, int placement, int* vertex_map, int memory,
                     fi_mesh** out);

/* ---- mesh smoothing: Taubin fairing, normals recomputed from the primitives -----------------------
 * Makes a device mesh smoother without the mesh leaving the device: Taubin's lambda | mu fairing with uniform ("umbrella")
 * weights (Taubin 1995; mu = 0: plain Laplacian smoothing), and vertex normals that fit the positions.  Any fi_mesh, 2-D
 * segments or 3-D triangles, with or without normals.  Both calls return a new immutable mesh with the input's vertex count,
 * keys and indices, copied (the keys stay ascending); nothing is kept with either handle.  The contract (DESIGN.md 4.16;
 * tests/smooth_reference.py is its definition in numpy) -- all arithmetic fp64 on the fp32 coordinates converted exactly, one
 * rounding per operation, every sum serial from 0 in the stated order:
 *   - half-edges: those of fi_mesh_parts ((a,b), (b,c), (c,a) of a triangle, (a,b) of a segment; equal ends are ignored).
 *     N(v): the distinct vertices a half-edge joins to v, in either direction, in ascending index order;
 *   - boundary.  3-D: a boundary edge is an unordered pair used by exactly one half-edge (fi_mesh_measure's `boundary`), a
 *     boundary vertex an end of one; an edge used three times or more, or twice in one direction, counts as interior.  2-D: a
 *     boundary vertex has total degree 1 (one half-edge touches it).  The set S(v) a vertex averages over:
 *       every mode                 N(v) empty (every unused vertex): S(v) empty;
 *       FI_SMOOTH_BOUNDARY_FIXED   boundary vertices: S(v) empty; others: N(v);
 *       FI_SMOOTH_BOUNDARY_SLIDE   3-D boundary vertices: B(v), the neighbours across v's boundary edges (ascending) -- a rim is
 *                                  faired as a curve and stays in a plane it lies in; others: N(v).  2-D: as FIXED;
 *       FI_SMOOTH_BOUNDARY_FREE    N(v) for every vertex.
 *     A vertex with empty S(v) never moves;
 *   - one step with factor f (lambda or mu as double), every vertex from the positions before the step (two buffers), per
 *     axis a: avg = (sum of x_w,a over w in S(v), ascending) / |S(v)|; t = avg - x_a; t = f t; x'_a = x_a + t;
 *   - one iteration: a lambda step; a mu step unless mu == 0; then, if max_move > 0, the clamp -- ONCE an iteration, behind
 *     its last step, not behind every step: d = x' - x0 per axis (x0 the input position), s2 = (d_x d_x + d_y d_y) + d_z d_z
 *     (2-D: the first two), m = max_move as double; if s2 > m m: x' = x0 + d (m / sqrt(s2)).  No vertex ends further than
 *     max_move from where it started (plus the rounding of the cast);
 *   - positions: (float)x after the last iteration; iterations == 0: the input's bytes;
 *   - normals.  FI_SMOOTH_NORMALS_KEEP: the input's, copied.  FI_SMOOTH_NORMALS_RECOMPUTE: those fi_mesh_normals gives for the
 *     output.  Either way a mesh without normals gives a mesh without normals.  fi_mesh_normals always gives normals (and
 *     the input's positions): for vertex v the primitives that reference v in ascending primitive number, one that names v
 *     twice counted once; n_p from the mesh's fp32 positions, 3-D (b - a) x (c - a) (n_x = u_y w_z - u_z w_y, ..., as in
 *     fi_mesh_simplify), 2-D (e_y, -e_x) with e = b - a -- not normalised (area / length weights), pointing from the
 *     extractors' inside to their outside; the sum divided by its length (sqrt of the squares summed in axis order), cast to
 *     fp32; a zero sum and an unused vertex give zeros;
 *   - an empty mesh: an empty mesh and FI_OK.  A NULL mesh, options or out; iterations < 0; lambda outside [0, 1], mu outside
 *     [-2, 0], max_move < 0, or any of them NaN; a bad boundary or normals code; a non-finite coordinate of a USED vertex
 *     (both calls; an unused vertex may hold anything and keeps it): FI_ERR_INVALID and no mesh.
 * No floating-point atomics and no atomics in the outputs: a repeated call returns the same bytes.  A vertex with very many
 * neighbours makes one thread sum them all: correct, and slow.  Not offered: cotangent or other geometry-dependent weights,
 * feature-preserving or bilateral filtering, implicit (solved) fairing, an adjacency cached with the handle, slab groups
 * (merge the pieces first: a seam is a boundary and stays jagged under FIXED), 1-D. */
#define FI_SMOOTH_BOUNDARY_FIXED 0
#define FI_SMOOTH_BOUNDARY_SLIDE 1
#define FI_SMOOTH_BOUNDARY_FREE  2
#define FI_SMOOTH_NORMALS_RECOMPUTE 0
#define FI_SMOOTH_NORMALS_KEEP      1
typedef struct fi_smooth_options {
	int   iterations;   /* >= 0 */
	float lambda, mu;   /* 0 <= lambda <= 1;  -2 <= mu <= 0;  mu == 0: no second step (plain Laplacian) */
	int   boundary;     /* FI_SMOOTH_BOUNDARY_* */
	float max_move;     /* > 0: no vertex ends further than this from where it started;  0: no limit */
	int   normals;      /* FI_SMOOTH_NORMALS_* */
} fi_smooth_options;
int fi_mesh_smooth(const fi_mesh* m, const fi_smooth_options* opt, fi_mesh** out);
int fi_mesh_normals(const fi_mesh* m, fi_mesh** out);

/* ---- points on a mesh, and how far one mesh lies from another surface ----------------------------
 * fi_mesh_sample spreads n points over a device mesh by area (2-D: by length), with normals and the primitive each lies on;
 * fi_mesh_deviation measures the distances of such points and of the mesh's vertices to a surface (fi_surface_*) and reduces
 * them to the same bytes on every run.  Any fi_mesh, 2-D segments or 3-D triangles.  The contract (DESIGN.md 4.17;
 * tests/meshpts_reference.py is its definition in numpy) -- all floating-point work fp64 on the fp32 coordinates converted
 * exactly, one rounding per operation; all integer work uint64, wrapping:
 *   - weights.  3-D: w_p = sqrt((n_x n_x + n_y n_y) + n_z n_z) of fi_mesh_normals' n_p = (b - a) x (c - a), its components formed
 *     as there; 2-D: w_p = sqrt(e_x e_x + e_y e_y), e = b - a.  A non-finite w_p counts as 0.  wmax = the largest w_p;
 *   - integer weights.  k = min(32, 52 - bits(np)), bits(np) the smallest b >= 1 with 2^b >= np;
 *     q_p = (uint64) floor((w_p / wmax) 2^k), 0 for every p when wmax = 0.  C = the inclusive prefix sums of q, T = their total
 *     (<= 2^52: exact as doubles).  A primitive with q_p = 0 is never sampled;
 *   - uniforms.  u(c) = (mix(seed + (c + 1) 0x9E3779B97F4A7C15) >> 11) 2^-53 with splitmix64's finaliser mix(z): z ^= z >> 30;
 *     z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.  Sample i draws xi = u(3 i), r1 = u(3 i + 1),
 *     r2 = u(3 i + 2) (2-D: the same counters, r2 unused);
 *   - stratum.  y = (((double)i + xi) / (double)n) (double)T; t = (uint64)y, T - 1 if t >= T; the primitive p = the number of
 *     entries of C that are <= t.  t never falls as i rises: the samples come out in ascending primitive order;
 *   - point.  3-D: if r1 + r2 > 1: r1 = 1 - r1, r2 = 1 - r2; per axis x = (a + r1 (b - a)) + r2 (c - a).  2-D: x = a + r1 (b - a).
 *     positions = (float)x;
 *   - normals.  FI_SAMPLE_NORMALS_FACE: n_p (2-D: (e_y, -e_x)) divided per component by w_p, pointing from the extractors'
 *     inside to their outside.  FI_SAMPLE_NORMALS_VERTEX: m = (w0 n_a + r1 n_b) + r2 n_c per axis from the mesh's vertex normals
 *     as doubles, w0 = (1 - r1) - r2 (2-D: w0 = 1 - r1, no n_c term), divided by its length (the squares summed in axis
 *     order); a zero or non-finite length: the face normal.  Both cast to fp32.
 * fi_mesh_sample: positions float[n][ndim] (required when n > 0), normals float[n][ndim] or NULL, primitives long long[n] or
 * NULL, all in `memory`.  n = 0: FI_OK, nothing written.  A NULL mesh, n < 0, NULL positions with n > 0, a bad mode or memory
 * kind, FI_SAMPLE_NORMALS_VERTEX with normals asked of a mesh that has none, T = 0 with n > 0 (an empty mesh, or nothing of
 * positive finite measure): FI_ERR_INVALID; n >= 2^31: FI_ERR_UNSUPPORTED.
 *
 * fi_mesh_deviation: two lists of queries against surface b -- the `samples` points of fi_mesh_sample(a, samples, seed), in
 * sample order (skipped when samples == 0 or of_samples is NULL; a mesh with nothing to sample: all of of_samples zero and
 * at = -1, no error), and the used vertices of a (those some primitive references), in ascending index order.  Every query's
 * d is what fi_surface_distance(b, ..., max_distance) returns for it.  A finite d is counted, +inf goes to `beyond`, NaN (a
 * non-finite vertex) to `invalid`.  max = the largest counted d, at = the first query that holds it, where = its position;
 * S1 = sum (double)d, S2 = sum (double)d (double)d over the list, uncounted entries contributing 0.0, both in a fixed order:
 * every block of 256 consecutive queries by the tree s[t] += s[t + w], w = 128, 64, ..., 1 (the tail padded with 0.0), the
 * block sums then added one after the other, ascending, from 0.0; mean = S1 / counted, rms = sqrt(S2 / counted); all three 0
 * when nothing is counted.  vertex_distances: float[a's vertex count] in `memory` or NULL, d for a used vertex and NaN for an
 * unused one.  The two structs are host memory.  NULL a or b; both structs and vertex_distances NULL; meshes of different
 * dimension or on different devices; samples < 0; a NaN or negative max_distance; a bad memory kind: FI_ERR_INVALID;
 * samples >= 2^31: FI_ERR_UNSUPPORTED.
 * No floating-point atomics and no atomics writing an output: a repeated call returns the same bytes.  Not offered: a walk
 * fused with the sampler, blue-noise or Poisson-disk spacing, per-vertex attribute transfer, slab groups (merge the pieces
 * first), 1-D. */
#define FI_SAMPLE_NORMALS_FACE   0
#define FI_SAMPLE_NORMALS_VERTEX 1
typedef struct fi_deviation {
	long long queries, counted, beyond, invalid, at;  /* at: the first query holding max; -1 when counted == 0 */
	double    max, mean, rms;
	float     where[3];                               /* that query's position (2-D: where[2] = 0) */
} fi_deviation;
int fi_mesh_sample(const fi_mesh* m, long n, unsigned long long seed, int normals_mode, float* positions, float* normals,
                   long long* primitives, int memory);
int fi_mesh_deviation(const fi_mesh* a, fi_surface* b, long samples, unsigned long long seed, float max_distance,
                      fi_deviation* of_samples, fi_deviation* of_vertices, float* vertex_distances, int memory);

/* ---- rigid registration of a point cloud to a mesh or to a point set (ICP) -----------------------
 * Finds the rotation R and translation t that lay n source points over a target -- a device mesh (its exact closest points,
 * fi_surface_distance) or a point set (fi_points_nearest) -- by iterated closest points, without the points leaving the
 * device.  ndim D = 2 or 3.  The contract (tests/register_reference.py is its definition in numpy) -- all
 * arithmetic fp64 on the fp32 inputs converted exactly, one rounding per operation, only + - * / sqrt (no sin, cos or atan:
 * device and host libm do not agree to the last bit), except where another contract is quoted.  The unknowns of a step are
 * delta = (omega, tau): 3-D (omega_0, omega_1, omega_2, tau_0, tau_1, tau_2), U = 6; 2-D (theta, tau_0, tau_1), U = 3:
 *   1. state.  R (D x D, row-major) and t (D) in double, from `initial` -- a (D + 1) x (D + 1) row-major double matrix on the
 *      HOST whose last row is ignored, taken as given and not checked for orthogonality -- or the identity.  The pivot
 *      g0_a = 0.5 ((double)lo_a + (double)hi_a) + 0.0 of the box of the finite source points (every coordinate finite; lo, hi
 *      the fp32 extremes, order-free; the + 0.0 makes a zero pivot +0).  No finite source point: zero iterations, g0 = 0,
 *      every point comes out `invalid`, FI_OK;
 *   2. transformed point.  p_i[a] = (float)(((R[a][0] x_0 + R[a][1] x_1) + R[a][2] x_2) + t[a]) (2-D: no third term); the
 *      current pivot g is the same expression of g0, kept in double;
 *   3. pair.  Mesh target: (d, prim, c) are exactly what fi_surface_distance(p, max_distance) returns.  Point-set target:
 *      (d, j) are exactly fi_points_nearest's and c is target point j.  A finite d is counted, +inf goes to `beyond`, NaN to
 *      `invalid`;
 *   4. normal (FI_REGISTER_PLANE only).  Mesh target: fi_mesh_normals' n_p of primitive prim (3-D (b - a) x (c - a), 2-D
 *      (e_y, -e_x)) divided per component by w_p = sqrt((n_0 n_0 + n_1 n_1) + n_2 n_2) (2-D: sqrt(e_x e_x + e_y e_y)).
 *      Point-set target: target_normals[j] as doubles divided by their length, the squares summed in axis order.  A length
 *      that is 0 or not finite: the pair goes to `degenerate`, uncounted;
 *   5. rows.  u = (double)p - g, e = (double)p - (double)c.
 *      PLANE, one row: r = (n_0 e_0 + n_1 e_1) + n_2 e_2; 3-D J = (u_1 n_2 - u_2 n_1, u_2 n_0 - u_0 n_2, u_0 n_1 - u_1 n_0, n_0,
 *      n_1, n_2); 2-D J = (u_0 n_1 - u_1 n_0, n_0, n_1); rho = |r|.
 *      POINT, D rows with r_a = e_a: 3-D J_0 = (0, u_2, -u_1, 1, 0, 0), J_1 = (-u_2, 0, u_0, 0, 1, 0), J_2 = (u_1, -u_0, 0, 0, 0,
 *      1); 2-D J_0 = (-u_1, 1, 0), J_1 = (u_0, 0, 1); rho = sqrt((e_0 e_0 + e_1 e_1) + e_2 e_2).
 *      The weight w is 1.0 with FI_LOSS_NONE; else fi_robust_reweight's three formulas in double with u = rho / sc,
 *      sc = (double)scale (double)c, c = tuning if > 0 else the fp32 constants 1.345f, 2.385f, 4.685f.
 *      A counted pair adds w (sum_a J_a[j] J_a[k]) to M[j][k] (j <= k), w (sum_a J_a[j] r_a) to b[j], w (sum_a r_a r_a) to S_w
 *      and sum_a r_a r_a to S; each inner sum runs over ascending a from its first term, zeros and ones included.  A pair
 *      that is not counted adds 0.0;
 *   6. sums over pairs.  Each of the U (U + 1) / 2 + U + 2 sums in fi_mesh_deviation's order: blocks of 256 consecutive
 *      source indices by the tree s[t] += s[t + w], w = 128 .. 1 (the tail padded with 0.0), the block sums then added
 *      ascending from 0.0.  The counts are integers;
 *   7. solve M delta = -b by Cholesky in the order of the unknowns, plain scalar operations.  top = the largest M[j][j] (top =
 *      M[0][0]; top = M[j][j] > top ? M[j][j] : top), lim = 1e-12 top.  For j ascending: d = M[j][j] - sum L[j][k] L[j][k] over
 *      the free k < j, subtracted one after the other in ascending k.  If not d > lim, unknown j is FIXED: delta_j = 0, it is
 *      skipped in every later sum and bit j of fixed_mask is set (bit 0 is omega_0 / theta).  Else L[j][j] = sqrt(d) and, for
 *      i > j, L[i][j] = (M[j][i] - sum L[i][k] L[j][k]) / L[j][j], the same way.  Forward: y_j = (-b[j] - sum L[j][k] y_k) /
 *      L[j][j], free k < j ascending, j ascending.  Back: delta_j = (y_j - sum L[k][j] delta_k) / L[j][j], free k > j
 *      DESCENDING from U - 1, j descending.  A plane may slide and a lone cylinder spin without a blow-up.  counted == 0:
 *      the loop stops and the step does not move the transform;
 *   8. update by the Cayley map: an exact rotation for any step, I + [omega]x to first order.  3-D: v = 0.5 omega,
 *      q = (v_0 v_0 + v_1 v_1) + v_2 v_2, den = 1 + q, c0 = 1 - q; R_d[a][a] = (c0 + 2 (v_a v_a)) / den;
 *      R_d[0][1] = (2 (v_0 v_1) - 2 v_2) / den, R_d[1][0] = (2 (v_0 v_1) + 2 v_2) / den, R_d[0][2] = (2 (v_0 v_2) + 2 v_1) / den,
 *      R_d[2][0] = (2 (v_0 v_2) - 2 v_1) / den, R_d[1][2] = (2 (v_1 v_2) - 2 v_0) / den, R_d[2][1] = (2 (v_1 v_2) + 2 v_0) / den.
 *      2-D: a = 0.5 theta, a2 = a a, den = 1 + a2, c = (1 - a2) / den, s = (2 a) / den, R_d = [[c, -s], [s, c]].  Then, from the
 *      old R, t and g: t'[a] = (((R_d[a][0] h_0 + R_d[a][1] h_1) + R_d[a][2] h_2) + g[a]) + tau[a] with h = t - g, and
 *      R'[a][b] = (R_d[a][0] R[0][b] + R_d[a][1] R[1][b]) + R_d[a][2] R[2][b];
 *   9. stop.  last_rotation = the largest |omega_j|, last_translation = the largest |tau_a| of the step just taken; the loop
 *      has converged when last_rotation <= rotation_tolerance and last_translation <= translation_tolerance, else it stops
 *      at max_iterations steps.  fixed_mask is the last step's.  A last evaluation then runs items 2 to 6 with no solve: it
 *      gives counted, beyond, invalid, degenerate, rms = sqrt(S / rows) and weighted_rms = sqrt(S_w / rows), rows = counted
 *      (PLANE) or D counted (POINT); both 0 when nothing is counted; `transformed` and `distances` are its p and d.
 *      max_iterations = 0 is this evaluation alone.  The fp32 rounding of p leaves a floor of about 1e-8 under the steps at
 *      coordinates near 10: tolerances under that floor are never met;
 *   10. result.  transform: the (D + 1) x (D + 1) matrix [R t; 0 1], row-major in the first (D + 1)^2 entries, the rest 0.
 * fi_mesh_register: `index` is a fi_surface of the target mesh, or NULL: built for the call.  `target` may be NULL with an
 * index and FI_REGISTER_POINT (a surface alone holds no vertices to take normals from).  fi_points_register:
 * target_normals float[m][ndim] in `memory` (m the set's points), NULL with FI_REGISTER_POINT.  source float[n][ndim],
 * transformed float[n][ndim] or NULL, distances float[n] or NULL, all in `memory`; options, initial and out are HOST.
 * n = 0: FI_OK, the identity or `initial` and zeros.  FI_ERR_INVALID: NULL target (and index), options or out; NULL source
 * with n > 0; n < 0; a mesh and an index of different dimension, device or primitive count; a 1-D point set;
 * max_iterations < 0; a NaN or negative max_distance or tolerance; a bad mode, loss or memory kind; a loss with scale <= 0 (a
 * median scale is not offered) or a NaN or negative tuning; a non-finite entry in the first D rows of `initial`;
 * FI_REGISTER_PLANE on a point set without normals or on a surface without its mesh.  n >= 2^31: FI_ERR_UNSUPPORTED.
 * Fewer than about 6 well-spread points leave the problem under-determined: the answer is then the caller's affair.
 * No atomics of any kind: a repeated call returns the same bytes.  Not offered: scale or affine fits, a median scale,
 * normal-compatibility rejection, source-side normals and symmetric ICP, global or coarse alignment (the caller supplies
 * `initial`), Levenberg damping, slab groups, 1-D, more than one target per call. */
#define FI_REGISTER_PLANE 0
#define FI_REGISTER_POINT 1
#define FI_LOSS_NONE (-1)
typedef struct fi_register_options {
	int    mode;             /* FI_REGISTER_* */
	int    max_iterations;   /* >= 0 */
	float  max_distance;     /* >= 0, may be +inf: pairs further apart are `beyond` */
	double rotation_tolerance, translation_tolerance;   /* >= 0 */
	int    loss;             /* FI_LOSS_NONE or FI_LOSS_HUBER / _CAUCHY / _TUKEY */
	float  tuning;           /* 0: the loss's default constant */
	float  scale;            /* > 0 with a loss */
} fi_register_options;
typedef struct fi_registration {
	double    transform[16];
	int       iterations, converged, fixed_mask, reserved;   /* reserved: 0 */
	long long queries, counted, beyond, invalid, degenerate;
	double    rms, weighted_rms, last_rotation, last_translation;
} fi_registration;
int fi_mesh_register(const fi_mesh* target, fi_surface* index, long n, const float* source, const fi_register_options* options,
                     const double* initial, fi_registration* out, float* transformed, float* distances, int memory);
int fi_points_register(const fi_points* target, const float* target_normals, long n, const float* source,
                       const fi_register_options* options, const double* initial, fi_registration* out, float* transformed,
                       float* distances, int memory);

/* ---- point queries: values and gradients at arbitrary positions --------------------------------
 * The contract ("Point queries") is this project's own:
 *   - positions: n points of ndim fp32 values, interleaved, in global lattice coordinates (x fastest, as fi_add_points);
 *     every axis needs size >= 2 (else FI_ERR_INVALID);
 *   - inside: every p_d finite and 0 <= p_d <= n_d - 1; an outside point gets `fill` for its value and every gradient
 *     component;
 *   - cell c_d = min((int)floor(p_d), n_d - 2), offset t_d = p_d - c_d in fp32 (exact, in [0, 1]: the upper face uses the
 *     last cell with t_d = 1);
 *   - FI_SAMPLE_LINEAR: u_d(0) = 1 - t_d, u_d(1) = t_d; corner i (bit d: +1 along axis d) weighs
 *     w_i = u_0(b_0) * u_1(b_1) * u_2(b_2), multiplied left to right -- for a point with every p_d < n_d - 1 these are the
 *     coefficients of the reference's add_value_constraint, bit for bit; value = sum over ascending i of w_i f_i; gradient
 *     component d = sum over ascending i with bit d clear of W_i^(not d) * (f_(i + 2^d) - f_i), W the product of the u_e,
 *     e != d, in ascending e (1 in 1-D).  Every sum starts from its first term;
 *   - FI_SAMPLE_CUBIC: samples c - 1 .. c + 2 along each axis, indices clamped to [0, n_d - 1]; Catmull-Rom
 *     a = p2 - p0, b = ((2 p0 - 5 p1) + 4 p2) - p3, e = (3 (p1 - p2) + p3) - p0, value p1 + (0.5 t) (a + t (b + t e)),
 *     derivative 0.5 (a + t (2 b + (3 t) e)); rows reduced along x, then y, then z; gradient component d takes the
 *     derivative along d and the value along the other axes;
 *   - fp32 with one rounding per operation; an FI_F64 context sampling its own solution computes in fp64 (t from the
 *     widened position) and rounds each output to fp32 once.  Non-finite field values propagate.
 * values: float[n]; gradients: float[n * ndim] or NULL; outputs in input order.  n = 0 is fine; n < 0, NULL positions or
 * values, a bad mode: FI_ERR_INVALID; n >= 2^31: FI_ERR_UNSUPPORTED.  `memory` applies to every buffer of the call.
 *
 * field: the context's owned values in fp32, or NULL for its last solution, read where it lives (FI_ERR_STATE before the first
 * solve).  On a slab context (nranks > 1, with its transport) the call is collective: every rank passes the same n and
 * positions and receives every point's result.  Each slab exchanges the ghost planes the mode reads (1 linear, 2 cubic;
 * FI_ERR_UNSUPPORTED where the context stores fewer, or a cubic call meets slabs thinner than 2 planes) and samples the
 * points whose slowest cell index c_(ndim-1) lies in its slab; the results are bit-identical to the undivided field's. */
int fi_sample(fi_ctx* ctx, const float* field, long n, const float* positions, int mode, float fill, float* values,
              float* gradients, int memory);
/* the same without a context: any whole field (e.g. the output of fi_upscale_field), fp32, x fastest */
int fi_sample_field(const float* field, int ndim, const int* sizes, long n, const float* positions, int mode, float fill,
                    float* values, float* gradients, int memory);

/* ---- nearest data points ------------------------------------------------------------------------
 * The contract ("Nearest data points") is this project's own:
 *   - the point set of a context: the positions of every fi_add_points batch in call order (fi_add_border_prior's rows are
 *     not data points); points outside the lattice count.  A point's index is its position in that concatenation.  A point
 *     with a non-finite coordinate is never nearest;
 *   - s(p, q): an fp32 sum from 0.0f of (p_d - q_d)^2 for d = 0, 1, 2 in ascending order, one rounding per operation (no FMA
 *     contraction) -- the arithmetic of the reference's border-prior loop;
 *   - a query q: best = the minimum of s over the finite points, distance = sqrtf(best), index = the smallest index with
 *     s == best.  No finite point: +inf and index -1; a query with a non-finite coordinate: NaN and index -1;
 *     sqrtf(best) > max_distance (>= 0, may be +inf): +inf and index -1;
 *   - results in input order: distances float[n], indices long long[n] (or NULL); they depend neither on the launch shape
 *     nor on timing.
 * n = 0 is fine.  n < 0, NULL queries or distances, a NaN or negative max_distance, a bad memory kind: FI_ERR_INVALID;
 * n >= 2^31 (queries or points): FI_ERR_UNSUPPORTED.  `memory` applies to every buffer of the call.
 *
 * A context builds its search structure at its first query and keeps it until the next fi_add_points or fi_clear_points.  A
 * slab context (nranks > 1) holds only the points near its slab: FI_ERR_UNSUPPORTED, as for fi_add_border_prior. */
int fi_nearest(fi_ctx* ctx, long n, const float* queries, float max_distance, float* distances, long long* indices, int memory);
/* every lattice point of the context (x fastest) as a query: out float[total], indices long long[total] or NULL */
int fi_distance_field(fi_ctx* ctx, float max_distance, float* out, long long* indices, int memory);

/* The same without a context: a point set of n positions (ndim = 1..3 floats each, interleaved, host or device), searched
 * on the current device.  A lattice of `sizes` (ndim extents >= 1, fewer than 2^31 points) for the distance field. */
int fi_points_create(fi_points** out, int ndim, long n, const float* positions, int memory);
int fi_points_nearest(fi_points* points, long n, const float* queries, float max_distance, float* distances, long long* indices,
                      int memory);
int fi_points_distance_field(fi_points* points, const int* sizes, float max_distance, float* out, long long* indices, int memory);
int fi_points_destroy(fi_points* points);

/* ---- k nearest data points ----------------------------------------------------------------------
 * The contract.  The point set, s(p, q), finiteness and max_distance are fi_nearest's, and so is the search
 * structure (built once, shared with fi_nearest):
 *   - a finite query q and 1 <= k <= 32: the pairs (s(p_j, q), j) over the finite points in lexicographic order (s first,
 *     then the index); the result is the first k of them with sqrtf(s) <= max_distance, in that order;
 *   - distances[i * k + r] = sqrtf(s_r), indices[i * k + r] = j_r; entries that do not exist (fewer than k finite points,
 *     neighbours beyond max_distance) are +inf / -1 and stand at the end;
 *   - a query with a non-finite coordinate: every distance NaN, every index -1;
 *   - a data point queried against its own set finds itself at distance 0 (or a duplicate with a smaller index first): it is
 *     not removed;
 *   - results depend neither on the launch shape nor on timing; for k = 1 they equal fi_nearest's bit for bit.
 * distances float[n * k], indices long long[n * k] or NULL.  The errors of fi_nearest; k outside 1..32: FI_ERR_INVALID. */
int fi_knn(fi_ctx* ctx, long n, const float* queries, int k, float max_distance, float* distances, long long* indices, int memory);
int fi_points_knn(fi_points* points, long n, const float* queries, int k, float max_distance, float* distances, long long* indices,
                  int memory);

/* ---- normals of a point cloud -------------------------------------------------------------------
 * The contract (tests/normals_reference.py is its definition in numpy).  For every point i of the set (a
 * context's points in the order they were added, or a fi_points), in ndim = 2 or 3 dimensions:
 *   1. its neighbours are its own fi_knn result (k, max_distance), itself included: m valid entries in result order.  A
 *      non-finite point, or m < ndim: the normal is all zeros and the variation NaN;
 *   2. everything else is fp64, one rounding per operation, only + - * / sqrt.  The centroid c: the neighbours' coordinates
 *      (widened from fp32) summed from 0.0 in neighbour order, divided by m.  The covariance sums: a_xy = the sum from 0.0 in
 *      neighbour order of (p_x - c_x)(p_y - c_y), not divided by m;
 *   3. six sweeps of a cyclic Jacobi iteration over the pairs (0,1), (0,2), (1,2) (2-D: the one pair), never fewer.  A pair
 *      with a_pq == 0 is skipped; else theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta theta + 1))
 *      with sign(0) = +1, c = 1 / sqrt(t t + 1), s = t c;  a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0;  the third axis r:
 *      (a_rp, a_rq) <- (c a_rp - s a_rq, s a_rp + c a_rq);  every row r of the vector matrix V (the identity at first):
 *      (v_rp, v_rq) <- (c v_rp - s v_rq, s v_rp + c v_rq);
 *   4. the normal is the column of V whose diagonal entry of A is smallest (the lowest column on a tie), its component of
 *      largest magnitude (the first such axis) made positive: the canonical sign.  variation = that diagonal entry / (the
 *      diagonal summed from 0.0 in axis order), 0 where that sum is 0: 0 on a plane, 1 / ndim for an isotropic neighbourhood;
 *   5. orient = FI_ORIENT_NONE: the canonical sign -- NOT a consistent orientation of the cloud.  FI_ORIENT_VIEWPOINTS:
 *      guides = num_guides viewpoints (1: one sensor position; or one per point); w = the sum from 0.0 in ascending axes of
 *      n_a (v_a - p_a), and the normal is negated where w < 0: normals look at the sensor, which is outward, the sign
 *      fi_add_points expects.  FI_ORIENT_DIRECTIONS: the same with guides[i] in place of v - p (rough normals from
 *      elsewhere), one per point.  w == 0 or non-finite: the canonical sign stays;
 *   6. normals float[n * ndim]: the fp64 components rounded to fp32, not renormalised; variation float[n] or NULL.
 * ndim = 1, k outside 1..32, k < ndim, NULL normals, a NaN or negative max_distance, a bad memory kind or orient, orient != 0
 * with NULL guides or a wrong num_guides: FI_ERR_INVALID.  A slab context: FI_ERR_UNSUPPORTED, as for fi_nearest.  `memory`
 * applies to every buffer of the call. */
enum { FI_ORIENT_NONE = 0, FI_ORIENT_VIEWPOINTS = 1, FI_ORIENT_DIRECTIONS = 2 };
int fi_estimate_normals(fi_ctx* ctx, int k, float max_distance, int orient, const float* guides, long num_guides, float* normals,
                        float* variation, int memory);
int fi_points_estimate_normals(fi_points* points, int k, float max_distance, int orient, const float* guides, long num_guides,
                               float* normals, float* variation, int memory);

/* ---- a consistent sign for the normals of a point cloud -------------------------------------------
 * The contract (tests/orient_reference.py is its definition in numpy).  `normals` float[n * ndim] in point
 * order (fi_estimate_normals' with FI_ORIENT_NONE, or any others) are read and written in place; ndim = 2 or 3:
 *   1. point i is LIVE if its position is finite and its normal is finite and not all zeros.  A point that is not live keeps
 *      its normal's bits and gets component -1;
 *   2. the graph: for every live i its own fi_knn result (k, max_distance) over the whole set; entries j = -1, j = i and j
 *      not live are skipped, every other entry is the undirected edge {i, j}; an edge listed from either side counts once;
 *   3. edge values, fp64 from the fp32 normals, one rounding per operation: d = 0.0 + n_i0 n_j0 + n_i1 n_j1 (+ n_i2 n_j2) in
 *      ascending axes (symmetric in i and j); flip = d < 0; a = (float)|d|;
 *   4. the edges are strictly ordered by (a descending, lo = min(i, j) ascending, hi = max(i, j) ascending): agreement of the
 *      normal LINES first, the indices make the order total.  The forest is the minimum spanning forest of the graph under
 *      that order -- unique, so the result does not depend on how it is computed;
 *   5. inside a component, t_i = +1 or -1 with t_i t_j = -1 exactly on the forest edges with flip, and t = +1 at the
 *      component's smallest point index c; components[i] = c (long long[n], or NULL);
 *   6. the component's sign S.  The extreme rule (FI_ORIENT_NONE, and a tied vote): e is the live member with the largest
 *      coordinate on the last axis (compared as fp32; a tie: the smallest index); of t_e n_e, from axis ndim - 1 down to 0,
 *      the first non-zero component decides: S = -1 if it is negative, else +1.  The vote (FI_ORIENT_VIEWPOINTS,
 *      FI_ORIENT_DIRECTIONS; guides as for fi_estimate_normals): w_i is step 5's expression of fi_estimate_normals for the
 *      normal t_i n_i; members with w > 0 vote +, with w < 0 vote -, with w == 0 or non-finite do not vote; more - than +:
 *      S = -1, more + than -: S = +1, equal counts: the extreme rule.  One sensor position thus serves a whole closed object,
 *      where fi_estimate_normals' per-point test is wrong on the far side;
 *   7. n_i <- S t_i n_i: the same bits, or every component's sign bit turned.
 * Results depend neither on the launch shape nor on timing.  ndim = 1, k outside 1..32, NULL normals, a NaN or negative
 * max_distance, a bad memory kind or anchor, anchor != 0 with NULL guides or a wrong num_guides: FI_ERR_INVALID.  A slab
 * context: FI_ERR_UNSUPPORTED.  n = 0 succeeds.  `memory` applies to every buffer of the call. */
int fi_orient_normals(fi_ctx* ctx, int k, float max_distance, int anchor, const float* guides, long num_guides, float* normals,
                      long long* components, int memory);
int fi_points_orient_normals(fi_points* points, int k, float max_distance, int anchor, const float* guides, long num_guides,
                             float* normals, long long* components, int memory);

/* ---- a point cloud made clean: thinning and outlier removal ---------------------------------------
 * The contract (tests/cloud_reference.py is its definition in numpy).  The point set, s(p, q), finiteness and
 * the search structure are fi_nearest's; ndim = 1, 2 or 3.  fp64 arithmetic is one rounding per operation over + - * / sqrt on
 * fp32 inputs converted exactly.  Every output is defined bit for bit and depends neither on the launch shape nor on timing.
 *
 * fi_radius_count: for a finite query, counts[i] = min(limit, the number of finite points j with sqrtf(s(p_j, q)) <= radius):
 * a point exactly on the radius counts; radius = +inf counts every finite point (one whose s overflows included).  A
 * non-finite query: -1.  queries float[n * ndim], counts int[n], both in `memory`.  The search stops at `limit` points: pass
 * the largest int for the exact number.  FI_ERR_INVALID: the errors of fi_nearest; a NaN or negative radius; limit < 1.
 *
 * fi_neighbour_distances: for point i of the set (a context's points in the order they were added, or a fi_points) and
 * 1 <= k <= 32: the pairs (s(p_j, p_i), j) over the finite points j != i in lexicographic order -- the point itself is left
 * out by its INDEX, a duplicate of it is a neighbour at distance 0; the first k of them with sqrtf(s) <= max_distance are its
 * neighbours, m of them.  mean[i] = (float)((0.0 + d_0 + ... + d_{m-1}) / m) with d_r = (double)sqrtf(s_r) added in result
 * order; kth[i] = sqrtf(s_{m-1}); counts[i] = m.  m = 0: mean and kth are +inf.  A non-finite point: NaN, NaN, 0.  mean
 * float[n], kth float[n], counts int[n] in `memory`; any of them may be NULL, not all three.  mean^ndim or kth^ndim is the
 * inverse local density: what a caller passes on as point weights.  FI_ERR_INVALID: k outside 1..32, a NaN or negative
 * max_distance, a bad memory kind, three NULL outputs.
 *
 * fi_outliers_statistical (the rule of PCL and Open3D): x_i = (double)mean[i] of fi_neighbour_distances(k, max_distance).
 * Point i is COUNTED iff x_i is finite; N = their number.  mu = T(x) / N, sigma = sqrt(T((x - mu)(x - mu)) / N), where T is
 * the fixed-order sum of fi_mesh_deviation over the array in POINT order, an uncounted point adding 0.0: blocks of 256
 * consecutive indices by the tree s[t] += s[t + w], w = 128 .. 1 (the tail padded with 0.0), the block sums then added
 * ascending from 0.0.  threshold = mu + (double)std_ratio sigma.  keep[i] = 1 iff i is counted and x_i <= threshold, else 0.
 * N = 0: nothing is kept, the doubles are 0, FI_OK.  keep unsigned char[n] in `memory` or NULL, stats on the HOST or NULL,
 * not both NULL.  FI_ERR_INVALID: as fi_neighbour_distances; a NaN or negative std_ratio.
 *
 * fi_outliers_radius: keep[i] = 1 iff p_i is finite and at least min_neighbours finite points j != i have
 * sqrtf(s(p_j, p_i)) <= radius.  keep unsigned char[n] in `memory` or NULL, *num_kept (HOST) or NULL, not both NULL.
 * FI_ERR_INVALID: a NaN or negative radius, min_neighbours < 1, a bad memory kind.
 *
 * The four above on a slab context: FI_ERR_UNSUPPORTED, as for fi_nearest.
 *
 * fi_cloud_thin: one output point per occupied cell of a uniform grid; it needs no search structure and runs on the current
 * device.  The cell of a finite point is fi_mesh_simplify's: c_a = floorf((p_a - o_a) / cell) in fp32, o = origin (HOST,
 * float[ndim]) or zeros, key = sum_a (c_a + 2^20) << 21 a.  A point with a non-finite coordinate is left out (cell_map -1): a
 * scan has such points.  Outputs are the occupied cells in ascending key order; a cell's members are taken in ascending
 * index, m of them.  FI_THIN_MEAN: position[a] = (float)((0.0 + p^0_a + p^1_a + ...) / m) in fp64; values (float[n], or NULL)
 * are averaged the same way; normals (float[n * ndim], or NULL): the fp64 sum S of the members' normals divided by
 * sqrt((S_0 S_0 + S_1 S_1) + S_2 S_2), all zeros where that length is not > 0.  FI_THIN_FIRST: position, normal and value of
 * the member with the lowest index, bit for bit.  Both: out_counts[c] = m (int), out_indices[c] = the lowest member's index
 * (long long), cell_map[i] = the output number of point i's cell (int).  Every output array has room for n entries and
 * *num_out (HOST) says how many were written; out_normals / out_values, out_counts, out_indices and cell_map may be NULL.
 * n = 0 or no finite point: *num_out = 0, FI_OK.  FI_ERR_INVALID: ndim outside 1..3, n < 0, NULL positions, out_positions or
 * num_out, out_normals without normals or out_values without values, a NaN or non-positive cell, a bad mode or memory kind, a
 * finite point with |c_a| >= 2^20.  n >= 2^31: FI_ERR_UNSUPPORTED.  A cell that holds the whole cloud is one thread's work:
 * slow and correct.
 * Not offered: lists of the neighbours within a radius, k > 32, a median / MAD threshold, slab contexts, approximate search
 * (smoothing of positions: fi_mls_project below). */
#define FI_THIN_MEAN  0
#define FI_THIN_FIRST 1
typedef struct fi_outlier_stats {
	long   counted, kept;
	double mean, stddev, threshold;
} fi_outlier_stats;
int fi_radius_count(fi_ctx* ctx, long n, const float* queries, float radius, int limit, int* counts, int memory);
int fi_points_radius_count(fi_points* points, long n, const float* queries, float radius, int limit, int* counts, int memory);
int fi_neighbour_distances(fi_ctx* ctx, int k, float max_distance, float* mean, float* kth, int* counts, int memory);
int fi_points_neighbour_distances(fi_points* points, int k, float max_distance, float* mean, float* kth, int* counts, int memory);
int fi_outliers_statistical(fi_ctx* ctx, int k, float max_distance, float std_ratio, unsigned char* keep, fi_outlier_stats* stats,
                            int memory);
int fi_points_outliers_statistical(fi_points* points, int k, float max_distance, float std_ratio, unsigned char* keep,
                                   fi_outlier_stats* stats, int memory);
int fi_outliers_radius(fi_ctx* ctx, float radius, int min_neighbours, unsigned char* keep, long* num_kept, int memory);
int fi_points_outliers_radius(fi_points* points, float radius, int min_neighbours, unsigned char* keep, long* num_kept, int memory);
int fi_cloud_thin(int ndim, long n, const float* positions, const float* normals, const float* values, float cell,
                  const float* origin, int mode, float* out_positions, float* out_normals, float* out_values, int* out_counts,
                  long long* out_indices, int* cell_map, long* num_out, int memory);

/* ---- a point cloud made smooth: moving-least-squares projection -------------------------------------
 * The contract (tests/mls_reference.py is its definition in numpy).  Every query is projected onto a plane
 * (degree 1) or a quadric (degree 2) fitted to its weighted neighbours, and gets that surface's normal and curvature.  The
 * point set, s(p, q), finiteness and the search structure are fi_nearest's; ndim = 2 or 3 (D below).  The queries are
 * `queries` (float[n * ndim]), or with queries == NULL the set's own points in point order (n is then not read: it is the
 * set's count).  Everything but s is fp64, one rounding per operation over + - * / sqrt on fp32 inputs converted exactly;
 * "the sum" of terms is 0.0 + the first + the second ..., in the order given.  h = (double)radius.  For a finite query q:
 *   1. neighbours: the first k pairs (s, j) of fi_knn's order (s ascending in fp32, equal s by ascending index) with
 *      sqrtf(s) <= radius, m of them, in that order -- "list order".  One of the set's own points finds itself (or a duplicate)
 *      first: it is a neighbour, as in fi_estimate_normals;
 *   2. weights: t = 1 - (double)s / (h h); t < 0 gives 0; w = (t t) t;
 *   3. W = the sum of w; the centroid c_a = (the sum of w x_a) / W; with e = x - c the covariance sums a_xy = the sum of
 *      (w e_x) e_y for x <= y, the other triangle copied, not divided by W; fi_estimate_normals' Jacobi iteration (step 3
 *      there) on it as it stands;
 *   4. the frame: n is the column of V whose diagonal entry of A is smallest (the lowest column on a tie), its component of
 *      largest magnitude (the first such axis) made positive; the tangents t1 (, t2) are the remaining columns in ascending
 *      column order, as they are.  Local coordinates of a point x: u = (the sum over ascending axes of e_a t1_a) / h, v
 *      likewise with t2 (3-D only), z likewise with n;
 *   5. refusal: m < D, or fewer than D weights > 0, or not W > 0: the point stays where it is -- order 0, position = q's bits,
 *      normal all zeros, curvature NaN;
 *   6. degree 2 and m >= NB, the basis b = (1, u, v, u u, u v, v v) in 3-D (NB = 6), (1, u, u u) in 2-D (NB = 3): the normal
 *      equations m_rs = the sum of (w b_r) b_s for r <= s, f_r = the sum of (w b_r) z.  Unpivoted Cholesky, columns j
 *      ascending: pivot d_j = m_jj - l_j0 l_j0 - ... - l_j,j-1 l_j,j-1, l_jj = sqrt(d_j), l_ij = (m_ji - l_i0 l_j0 - ... -
 *      l_i,j-1 l_j,j-1) / l_jj for i > j ascending; y_i = (f_i - l_i0 y_0 - ... - l_i,i-1 y_i-1) / l_ii ascending;
 *      x_i = (y_i - l_i+1,i x_i+1 - ... - l_NB-1,i x_NB-1) / l_ii descending.  If every d_j > 1e-15 W the coefficients are x
 *      and order = 2; else, and for degree 1 or m < NB, they are all 0.0 and order = 1 (the plane);
 *   7. projection, (u0, v0) the local coordinates of q.  3-D: p = ((((x0 + x1 u0) + x2 v0) + x3 (u0 u0)) + x4 (u0 v0)) +
 *      x5 (v0 v0); pu = (x1 + (2 x3) u0) + x4 v0; pv = (x2 + x4 u0) + (2 x5) v0; x'_a = c_a + h ((u0 t1_a + v0 t2_a) + p n_a);
 *      g_a = (n_a - pu t1_a) - pv t2_a; A = 1 + pu pu, B = 1 + pv pv, G = A + pv pv; curvature = ((B (2 x3) - ((2 pu) pv) x4) +
 *      A (2 x5)) / ((2 h) (G sqrt(G))): the mean curvature of the graph, in 1 / length, positive where the surface bends
 *      towards the normal.  2-D: p = (x0 + x1 u0) + x2 (u0 u0); pu = x1 + (2 x2) u0; x'_a = c_a + h (u0 t1_a + p n_a);
 *      g_a = n_a - pu t1_a; G = 1 + pu pu; curvature = (2 x2) / (h (G sqrt(G))).  order 1: curvature = 0.0.  The normal is
 *      g / sqrt(g_0 g_0 + g_1 g_1 (+ g_2 g_2));
 *   8. guide_normals (float[n * ndim], one per query, or NULL): d = the sum over ascending axes of normal_a (double)guide_a; d
 *      finite and < 0 negates the normal and the curvature: normals oriented by fi_orient_normals come back oriented;
 *   9. max_move (>= 0; +inf: no limit), fi_mesh_smooth's rule: dl = x' - q, s2 = dl_0 dl_0 + dl_1 dl_1 (+ dl_2 dl_2); if
 *      s2 > max_move max_move then x' = q + dl (max_move / sqrt(s2));
 *  10. a non-finite x', normal or curvature: the outputs of step 5.  Otherwise positions, normals and curvature are the fp64
 *      figures rounded to fp32.
 * A non-finite query: position all NaN, order 0, normal zeros, curvature NaN.  A non-finite point of the set (queries ==
 * NULL): its position's bits as they were given, order 0, normal zeros, curvature NaN.
 * positions float[n * ndim], normals float[n * ndim], curvature float[n], order unsigned char[n]: any of them may be NULL,
 * not all four.  Results depend neither on the launch shape nor on timing.  The plane shrinks a curved surface (a sphere of
 * radius R by about the squared neighbourhood size over R); the quadric does not, but with few neighbours for its six
 * coefficients (k = 16 on a noisy surface) it amplifies noise: keep k = 32 for degree 2.  The set's points are not moved: to go
 * on with the smoothed cloud, build a new point set from `positions`.
 * FI_ERR_INVALID: ndim = 1, k outside 1..32, a radius that is not > 0 and finite, a degree other than 1 or 2, a NaN or negative
 * max_move, four NULL outputs, a bad memory kind, n < 0.  n >= 2^31: FI_ERR_UNSUPPORTED.  A slab context: FI_ERR_UNSUPPORTED,
 * as for fi_nearest.  `memory` applies to every buffer of the call.
 * Not offered: Gaussian weights, degree above 2, k > 32, iterated projection (call again on a new set), upsampling beyond
 * caller-supplied queries, slab contexts. */
int fi_mls_project(fi_ctx* ctx, long n, const float* queries, int k, float radius, int degree, float max_move,
                   const float* guide_normals, float* positions, float* normals, float* curvature, unsigned char* order, int memory);
int fi_points_mls_project(fi_points* points, long n, const float* queries, int k, float radius, int degree, float max_move,
                          const float* guide_normals, float* positions, float* normals, float* curvature, unsigned char* order,
                          int memory);

/* ---- the clusters of a point cloud: Euclidean clusters and DBSCAN ------------------------------------
 * The contract (tests/cluster_reference.py is its definition in numpy).  The point set, s(p, q), finiteness
 * and the search structure are fi_nearest's; "within eps" is fi_radius_count's rule, sqrtf(s(p_j, p_i)) <= eps: a pair exactly
 * at eps is joined.  ndim = 1, 2 or 3.  Every output is defined bit for bit and depends neither on the launch shape nor on
 * timing.
 *
 * fi_cluster labels the set's own points (a context's points in the order they were added, or a fi_points):
 *   - CORE: a finite point i is core iff at least min_points finite points j have sqrtf(s(p_j, p_i)) <= eps.  The count
 *     includes i itself (the count of sklearn and Open3D); a duplicate of i counts as another point.  min_points = 1 makes
 *     every finite point core: plain Euclidean clustering (PCL's EuclideanClusterExtraction).
 *   - CLUSTERS: two core points within eps of each other are joined; the clusters are the connected components of that graph
 *     over the core points, numbered 0, 1, ... in ascending order of each cluster's LOWEST CORE POINT INDEX.
 *   - BORDER: a finite point that is not core and has a core point within eps takes the cluster of its nearest one: of the
 *     first pair (s, j) in lexicographic order over the core points j -- fi_nearest's tie rule restricted to core points.
 *     (Classic DBSCAN's "whichever cluster reaches it first" depends on the order of the visit; this rule does not.)  A
 *     border point joins nothing else to anything.
 *   - NOISE: every other finite point gets the label -1; so does a non-finite point.
 * labels int[n] in `memory`; core unsigned char[n] in `memory` (1 for a core point) or NULL; stats on the HOST or NULL; not
 * both labels and stats NULL.  stats: clusters, and the numbers of core, border, noise (finite, label -1) and non-finite
 * points, which add up to n.  n = 0 or no finite point: zero clusters, FI_OK.  FI_ERR_INVALID: a NaN, negative or infinite
 * eps; min_points < 1; a bad memory kind; labels and stats both NULL.  A slab context: FI_ERR_UNSUPPORTED, as for the four
 * cleaning calls.  Cost: an eps that reaches across the whole cloud makes every thread visit every point: slow and correct.
 *
 * fi_cluster_measure: one row per cluster of a labelling; it needs no search structure and runs on the current device.
 * positions float[n * ndim], labels int[n] and core unsigned char[n] (or NULL) in `memory`; rows on the HOST, num_clusters of
 * them.  The members of cluster c are the points with label c.  count and core (the members whose core byte is not 0; 0
 * with core = NULL) are exact; lo / hi are the fp32 minimum / maximum of the members' coordinates; centroid[a] takes the
 * members in ascending index, cut into chunks of 256 consecutive members: each chunk is summed in fp64 by fi_mesh_deviation's
 * fixed tree (s[t] += s[t + w], w = 128 .. 1, the tail padded with 0.0), the chunk sums are added ascending from 0.0 and the
 * total is divided by count.  Unused axes are 0; a cluster without a member is a row of zeros.  A cluster of a million
 * points costs one thread 4096 additions.  FI_ERR_INVALID: ndim outside 1..3, n or num_clusters < 0, NULL positions or labels
 * with n > 0, NULL rows with num_clusters > 0, a bad memory kind, a label outside [-1, num_clusters).  n or num_clusters
 * >= 2^31: FI_ERR_UNSUPPORTED.
 * Not offered: lists of the neighbours within a radius, HDBSCAN, OPTICS, region growing by normals, slab contexts,
 * approximate search. */
typedef struct fi_cluster_stats {
	long clusters, core, border, noise, non_finite;
} fi_cluster_stats;
typedef struct fi_cluster_row {
	long   count, core;
	float  lo[3], hi[3];
	double centroid[3];
} fi_cluster_row;
int fi_cluster(fi_ctx* ctx, float eps, int min_points, int* labels, unsigned char* core, fi_cluster_stats* stats, int memory);
int fi_points_cluster(fi_points* points, float eps, int min_points, int* labels, unsigned char* core, fi_cluster_stats* stats,
                      int memory);
int fi_cluster_measure(int ndim, long n, const float* positions, const int* labels, const unsigned char* core, long num_clusters,
                       fi_cluster_row* rows, int memory);

/* ---- the dominant hyperplanes of a point cloud: RANSAC with refits ------------------------------
 * The contract (tests/plane_reference.py is its definition in numpy) is this project's own.  fi_plane_fit
 * fits one hyperplane n . x + d = 0 (a plane in 3-D, a line in 2-D; ndim = 1: FI_ERR_INVALID) to positions float[n * ndim];
 * fi_planes_segment peels several off, one after the other.  No search structure: positions, mask, inliers and labels lie
 * in `memory`, the models on the HOST; the calls run on the current device.  Everything is fp64 computed from the fp32
 * coordinates, one rounding per operation (no FMA contraction), over + - * / sqrt; there are no float atomics, and every
 * output is defined bit for bit, whatever the launch shape and the timing.
 *   - candidates: point i is one iff all its coordinates are finite and mask is NULL or mask[i] != 0; in ascending index
 *     they form the list cand[0 .. m).  m < ndim: found = 0, trials = 0;
 *   - hypothesis h = 0 .. max_trials - 1 draws D = ndim list positions j_k = min(floor(u(seed, h D + k) m), m - 1), u being
 *     fi_mesh_sample's counter hash (splitmix64's finaliser of seed + (counter + 1) 0x9E3779B97F4A7C15, its top 53 bits times
 *     2^-53).  With a, b, c the drawn points: 3-D n = (b - a) x (c - a), each component the difference of two products
 *     (u_1 w_2 - u_2 w_1, u_2 w_0 - u_0 w_2, u_0 w_1 - u_1 w_0); 2-D t = b - a, n = (-t_1, t_0).  len = sqrt of the squares
 *     summed over ascending axes; n = n / len; d = -(n_0 a_0 + n_1 a_1 (+ n_2 a_2)), summed over ascending axes.  The
 *     hypothesis is invalid when two of its j_k are equal or when len is not finite and > 0; with an axis constraint
 *     (min_cos > 0), t = the sum over ascending axes of n_a axis_a, also when t t >= (min_cos min_cos) (axis . axis) is false.
 *     An invalid hypothesis scores -1;
 *   - score: e_i = ((n_0 x_0 + n_1 x_1) + n_2 x_2) + d (2-D: (n_0 x_0 + n_1 x_1) + d); candidate i is an inlier iff
 *     fabs(e_i) <= (double)threshold -- a point exactly at the threshold is in.  The score is the exact count of inliers among
 *     the candidates; the best hypothesis has the highest score, ties go to the lowest h; no valid hypothesis: found = 0;
 *   - batches and the stop: hypotheses are scored in batches of FI_PLANE_BATCH, the last may be partial.  After every batch,
 *     with T the hypotheses scored so far and b > 0 the best score: w = b / m, p = w w (times w again in 3-D), q = 1 - p, and
 *     r = q^T by binary exponentiation from the low bit (r = 1; base = q; while (e) { if (e & 1) r = r base; base = base base;
 *     e >>= 1; }), all in fp64: stop when r <= 1 - confidence.  No logarithm: add, multiply and compare only.  confidence = 0
 *     never stops early.  trials reports T;
 *   - refits, `refine` times: the members are the current inliers in ascending index; c_a = tree_sum(x_a) / count;
 *     A_ab = tree_sum((x_a - c_a)(x_b - c_b)) for a <= b, mirrored; tree_sum is fi_cluster_measure's (chunks of 256
 *     consecutive members, s[t] += s[t + w], w = 128 .. 1, the tail padded with 0.0; the chunk sums added ascending from 0.0);
 *     fi_estimate_normals' cyclic Jacobi iteration (6 sweeps); the new normal is the column with the smallest diagonal entry,
 *     the lowest column on a tie, NOT renormalised; d = -(n_0 c_0 + ...).  The inliers are then counted again over all
 *     candidates.  A refit is skipped, and the refits end, when count < D or the new normal is not finite.  A refit is not
 *     conditional on the count going up.  refits reports how many ran;
 *   - result: the final normal takes fi_estimate_normals' canonical sign (the component of largest magnitude, the first such
 *     axis, is positive), offset is negated with it; rms = sqrt(tree_sum(e^2) / inliers) over the final inliers, 0 with none;
 *     inliers (unsigned char[n] or NULL) is one byte per input point from the final model.  Unused axes of normal are 0;
 *     found = 0 leaves every figure but candidates and trials 0.
 * fi_planes_segment: plane p is fi_plane_fit with seed + p (wrapping) over the candidates no earlier plane took; the loop
 * ends at max_planes, at found = 0, or at the first plane with fewer than min_inliers inliers, which is not recorded.
 * labels[i] (int[n]) is the plane that took point i, or -1; rows (host, max_planes) receive the recorded models and
 * *num_planes their number.  n = 0: found = 0, no planes, FI_OK.
 * FI_ERR_INVALID: ndim outside 2..3; n < 0; a negative, NaN or infinite threshold; max_trials outside 1 .. 2^20; confidence
 * outside [0, 1); refine outside 0 .. 16; min_cos outside [0, 1]; min_cos > 0 with a zero or non-finite axis; a bad memory
 * kind; NULL required pointers (opt, model / labels, rows, num_planes; positions with n > 0); max_planes < 1;
 * min_inliers < 0.  n >= 2^31: FI_ERR_UNSUPPORTED.
 * Spheres, cylinders and per-point normals in the inlier test: fi_shape_fit / fi_shapes_segment below.
 * Not offered: cones, tori and other models; MSAC / MLESAC scores; region growing by normals; slab contexts. */
#define FI_PLANE_BATCH 1024
typedef struct fi_plane_options {
	float              threshold;
	long               max_trials;
	double             confidence;
	int                refine;
	unsigned long long seed;
	float              axis[3];
	float              min_cos;
} fi_plane_options;
typedef struct fi_plane_model {
	int    found, refits;
	long   inliers, candidates, trials;
	double normal[3], offset, rms;
} fi_plane_model;
int fi_plane_fit(int ndim, long n, const float* positions, const unsigned char* mask, const fi_plane_options* opt,
                 fi_plane_model* model, unsigned char* inliers, int memory);
int fi_planes_segment(int ndim, long n, const float* positions, const unsigned char* mask, const fi_plane_options* opt,
                      int max_planes, long min_inliers, int* labels, fi_plane_model* rows, int* num_planes, int memory);

/* ---- the spheres and cylinders of a point cloud: RANSAC with refits ------------------------------
 * The contract (tests/shape_reference.py is its definition in numpy) is this project's own.  fi_shape_fit
 * fits one shape of opt->kind to positions float[n * ndim]: FI_SHAPE_SPHERE a sphere |x - c| = r (a circle with ndim = 2),
 * FI_SHAPE_CYLINDER a cylinder |(x - q) - ((x - q) . a) a| = r (ndim = 3 only); fi_shapes_segment peels several off, one after
 * the other.  normals float[n * ndim] may be NULL for a sphere; a cylinder's hypotheses and refits are made of them.
 * positions, normals, mask, inliers and labels lie in `memory`, the models on the HOST; the calls run on the current device.
 * Everything is fp64 computed from the fp32 inputs, one rounding per operation (no FMA contraction), over + - * / sqrt, fabs
 * and compares; there are no float atomics, and every output is defined bit for bit, whatever the launch shape and the
 * timing.  a . b is the sum of the products over ascending axes.
 *   - candidates: point i is one iff all its coordinates are finite, mask is NULL or mask[i] != 0 and, where normals are
 *     passed, every component of its normal is finite and len = sqrt(n . n) is finite and > 0 (fi_points_describe's length);
 *     its unit normal is u = n / len per component.  In ascending index they form the list cand[0 .. m).  With S = 4 (sphere,
 *     3-D), 3 (circle) or 2 (cylinder) the points a hypothesis draws: m < S gives found = 0, trials = 0;
 *   - hypothesis h = 0 .. max_trials - 1 draws S list positions j_k = min(floor(u(seed, h S + k) m), m - 1) by fi_plane_fit's
 *     counter hash; p_k and u_k are the drawn points and their unit normals.
 *     Sphere: q_k = p_k - p_0 and h_k = 0.5 (q_k . q_k) for k = 1 .. D; c' solves M c' = h, M's rows being the q_k, by
 *     Cramer's rule: 2-D det = M00 M11 - M01 M10, x_0 = (M11 h_0 - M01 h_1) / det, x_1 = (M00 h_1 - M10 h_0) / det; 3-D the
 *     cofactors C_ij = M_i'j' M_i"j" - M_i'j" M_i"j' with i' = (i + 1) mod 3, i" = (i + 2) mod 3 (and so j), det =
 *     (M00 C00 + M01 C01) + M02 C02, x_j = ((C0j h_0 + C1j h_1) + C2j h_2) / det.  Invalid when det is not finite or is 0.
 *     c = p_0 + c', r = sqrt(c' . c').
 *     Cylinder: a = u_0 x u_1, each component the difference of two products (u0_1 u1_2 - u0_2 u1_1, u0_2 u1_0 - u0_0 u1_2,
 *     u0_0 u1_1 - u0_1 u1_0); len = sqrt(a . a), invalid unless finite and > 0; a = a / len.  d = p_1 - p_0, g00 = u_0 . u_0,
 *     g01 = u_0 . u_1, g11 = u_1 . u_1, b0 = u_0 . d, b1 = u_1 . d, det = g00 g11 - g01 g01, invalid unless finite and != 0;
 *     s = (b0 g11 - g01 b1) / det; the axis point q = p_0 + s u_0 per component; r = fabs(s).
 *     Both: invalid when two of the j_k are equal, and unless r is finite and (double)r_min <= r <= (double)r_max (r_max =
 *     +inf: no upper limit).  An invalid hypothesis scores -1;
 *   - band, once a model: lo = r - (double)threshold, 0 where that is not > 0; lo2 = lo lo; hi = r + threshold; hi2 = hi hi;
 *   - score, no square root: sphere g = x - c; cylinder v = x - q, t = v . a, g = v - t a; s_i = g . g.  Candidate i is an
 *     inlier iff lo2 <= s_i <= hi2 -- a point exactly on either edge is in -- and, with normal_cos > 0, also s_i > 0 and
 *     (u_i . g)^2 >= (mc mc) s_i, mc = (double)normal_cos: the point's normal lies within that angle of the shape's, either
 *     way round.  The score is the exact count; ties, the batches of FI_SHAPE_BATCH, the stop rule (with this S as the
 *     exponent: p = w multiplied by w S - 1 times), trials and candidates are fi_plane_fit's;
 *   - refits, `refine` times, over the current inliers in ascending index, every sum fi_plane_fit's tree_sum:
 *     m_a = tree_sum(x_a) / count, y = x - m.  Sphere (Kasa), in F = D dimensions: w = y . y; the sums A_ab = tree_sum(y_a y_b)
 *     (a <= b, mirrored), B_a = tree_sum(y_a w), W = tree_sum(w); c' solves A c' = 0.5 B by the Cramer routine above;
 *     c = m + c'; r = sqrt(c' . c' + W / count).  Cylinder: N_ab = tree_sum(u_a u_b) of the members' unit normals (a <= b,
 *     mirrored, not centred); fi_estimate_normals' Jacobi iteration (6 sweeps) of N; the new axis is the column with the
 *     smallest diagonal entry, the lowest column on a tie, NOT renormalised; e_1, e_2 are the other two columns in ascending
 *     column order; then the same Kasa sums in F = 2 dimensions over f = (y . e_1, y . e_2), their solution (c_u, c_v),
 *     q = (m + c_u e_1) + c_v e_2 per component, r = sqrt((c_u c_u + c_v c_v) + W / count).  The inliers are then counted
 *     again over all candidates.  A refit is skipped, and the refits end, when count < S + 1, the determinant is not finite
 *     or is 0, a figure of the new model or of the frame is not finite, or the new r leaves [r_min, r_max].  A refit is not
 *     conditional on the count going up.  refits reports how many ran;
 *   - result: center is c (sphere; unused axes 0) or q (cylinder); radius is r; axis is a with fi_estimate_normals' canonical
 *     sign (the component of largest magnitude, the first such axis, is positive), zeros for a sphere; extent is the least
 *     and the greatest (x - q) . axis over the final inliers (zeros for a sphere or with none); rms =
 *     sqrt(tree_sum((sqrt(s_i) - r)^2) / inliers), 0 with none; inliers (unsigned char[n] or NULL) is one byte per input
 *     point from the final model; kind repeats opt->kind.  found = 0 leaves every figure but candidates and trials 0.
 * fi_shapes_segment: shape p is fi_shape_fit with seed + p (wrapping) over the candidates no earlier shape took; the loop ends
 * at max_shapes, at found = 0, or at the first shape with fewer than min_inliers inliers, which is not recorded.  labels[i]
 * (int[n]) is the shape that took point i, or -1; rows (host, max_shapes) receive the recorded models and *num_shapes their
 * number.  n = 0: found = 0, no shapes, FI_OK.
 * FI_ERR_INVALID: ndim outside 2..3; n < 0; an unknown kind; a cylinder without normals; a negative, NaN or infinite
 * threshold; r_min < 0; r_max < r_min; a NaN limit; normal_cos outside [0, 1]; normal_cos > 0 without normals; max_trials
 * outside 1 .. 2^20; confidence outside [0, 1); refine outside 0 .. 16; a bad memory kind; NULL required pointers (opt,
 * model / labels, rows, num_shapes; positions with n > 0); max_shapes < 1; min_inliers < 0.  FI_ERR_UNSUPPORTED: a cylinder
 * with ndim = 2; n >= 2^31.
 * Not offered: cones and tori; a radius-weighted or geometric (non-algebraic) refit; MSAC / MLESAC scores; slab contexts. */
#define FI_SHAPE_SPHERE   0      /* a circle when ndim = 2 */
#define FI_SHAPE_CYLINDER 1      /* 3-D only */
#define FI_SHAPE_BATCH    1024
typedef struct fi_shape_options {
	int                kind;
	float              threshold;
	float              r_min, r_max;
	float              normal_cos;
	long               max_trials;
	double             confidence;
	int                refine;
	unsigned long long seed;
} fi_shape_options;
typedef struct fi_shape_model {
	int    found, kind, refits;
	long   inliers, candidates, trials;
	double center[3], axis[3], radius, extent[2], rms;
} fi_shape_model;
int fi_shape_fit(int ndim, long n, const float* positions, const float* normals, const unsigned char* mask,
                 const fi_shape_options* opt, fi_shape_model* model, unsigned char* inliers, int memory);
int fi_shapes_segment(int ndim, long n, const float* positions, const float* normals, const unsigned char* mask,
                      const fi_shape_options* opt, int max_shapes, long min_inliers, int* labels, fi_shape_model* rows,
                      int* num_shapes, int memory);

/* ---- descriptors of a point's neighbourhood that survive a rigid motion, and their matching -----
 * The contract (tests/feature_reference.py is its definition in numpy) is this project's own: Rusu's fast
 * point feature histograms with a pseudo-angle in place of the third feature's angle, so that no trigonometry is needed.
 * fi_points_describe gives every point of a 3-D set (any other ndim: FI_ERR_UNSUPPORTED) FI_FEATURE_WIDTH = 33 floats from
 * its k nearest points and the normals float[n * 3]; features float[n * 33] and valid unsigned char[n] (or NULL) lie in
 * `memory` like the normals.  Everything is fp64 computed from the fp32 positions and normals, one rounding per operation (no
 * FMA contraction), over + - * / sqrt, fabs and compares; counts are integers; every output is defined bit for bit.
 *   - live: point i is live iff its position is finite and its normal is finite with a length -- the square root of the
 *     squares summed over ascending axes in double, (x_0^2 + x_1^2) + x_2^2 -- that is finite and > 0.  Its unit normal is
 *     n = (double)normal / length per component.  A point that is not live gets 33 zeros and valid = 0;
 *   - neighbours: the neighbours of a live point i are its own fi_points_knn result (k, max_distance) over the whole set, in
 *     result order, without the entries j = -1, j = i, j not live and j with w = 0 (below);
 *   - pair (i, j): dp = p_j - p_i; w = (dp_0^2 + dp_1^2) + dp_2^2, L = sqrt(w), e = dp / L; a_i = n_i . e and a_j = n_j . e,
 *     every dot product (u_0 v_0 + u_1 v_1) + u_2 v_2.  If fabs(a_i) < fabs(a_j): (n_s, n_t, e, f_2) = (n_j, n_i, -e, -a_j),
 *     else (n_i, n_j, e, a_i) -- PCL's choice of the source as the point whose normal lies closer to the line, without acos.
 *     v = e x n_s, each component the difference of two products (e_1 n_2 - e_2 n_1, e_2 n_0 - e_0 n_2, e_0 n_1 - e_1 n_0);
 *     l = sqrt of its squares summed as above; the pair is skipped unless l is finite and > 0; v = v / l; u = n_s x v;
 *     f_1 = v . n_t, x = n_s . n_t, y = u . n_t; s = fabs(x) + fabs(y), r = s > 0 ? y / s : 0; the pseudo-angle
 *     f_3 = x >= 0 ? r : (y >= 0 ? 2 - r : -2 - r), in [-2, 2], monotone in atan2(y, x).  A pair with a non-finite f is skipped;
 *   - bins, 11 per feature: t_1 = (f_1 + 1) 5.5, t_2 = (f_2 + 1) 5.5, t_3 = (f_3 + 2) 2.75; b = t < 0 ? 0 : t >= 11 ? 10 :
 *     (int)t; c_i[b_1], c_i[11 + b_2], c_i[22 + b_3] and the pair count m_i each gain 1;
 *   - SPFH: S_i[b] = (100.0 c_i[b]) / m_i for a live i with m_i > 0; any other point has no descriptor: zeros, valid = 0;
 *   - FPFH: over the same neighbours in the same order, only those with m_j > 0 (q_i of them): A[b] = the sum from 0.0 of
 *     S_j[b] / w_ij; F[b] = S_i[b] + (q_i > 0 ? A[b] / q_i : 0); per block of 11: z = the sum from 0.0 over its ascending bins,
 *     F[b] = (100.0 F[b]) / z where z > 0; features[i 33 + b] = (float)F[b], valid[i] = 1.
 * FI_ERR_INVALID: a NULL set, normals or features; k outside 1..32; a negative or NaN max_distance; a bad memory kind.  An
 * empty set succeeds.
 * fi_feature_match: for every row i of a (float[n_a * dim], 1 <= dim <= FI_FEATURE_MAX_DIM), over the rows j of b
 * (float[n_b * dim]) that are valid (valid_b NULL or valid_b[j] != 0) and finite: s(i, j) = the fp32 sum from 0.0f of
 * (a_ic - b_jc)^2 over ascending c, one rounding per operation.  indices[i] (long long[n_a]) is the smallest j with the
 * minimal s, distances[i] (float[n_a] or NULL) = sqrtf(s); an invalid or non-finite row i, or no admissible j: -1 and +inf.
 * All buffers in `memory`, on the current device.  FI_ERR_INVALID: dim outside 1..64; a negative count; NULL a or indices
 * with n_a > 0, NULL b with n_a > 0 and n_b > 0; a bad memory kind.  n_a or n_b >= 2^31: FI_ERR_UNSUPPORTED.
 * Not offered: 2-D; fi_ctx entries; neighbourhoods by radius, k > 32; approximate descriptor search; matrix-core matching
 * (the contract fixes the order of the sum); slab contexts. */
#define FI_FEATURE_WIDTH 33
#define FI_FEATURE_MAX_DIM 64
int fi_points_describe(fi_points* points, const float* normals, int k, float max_distance, float* features, unsigned char* valid,
                       int memory);
int fi_feature_match(int dim, long n_a, const float* a, const unsigned char* valid_a, long n_b, const float* b,
                     const unsigned char* valid_b, long long* indices, float* distances, int memory);

/* ---- the rigid motion that most matched pairs agree on: RANSAC over correspondences --------------
 * The contract (tests/align_reference.py is its definition in numpy) is this project's own.
 * fi_align_correspondences finds the rotation and shift x -> R x + t that carries the most source points of the matched pairs
 * (source[src_index[c]], target[tgt_index[c]]), c = 0 .. m - 1, to within `threshold` of their target points: the coarse
 * alignment from any pose whose result fi_points_register takes as `initial`.  3-D only: source is float[n_s * 3], target
 * float[n_t * 3].  No search structure: the points, the indices (long long[m]) and inliers (unsigned char[m] or NULL) lie in
 * `memory`, out on the HOST; the call runs on the current device.  Everything is fp64 computed from the fp32 coordinates, one
 * rounding per operation (no FMA contraction), over + - * / sqrt; there are no float atomics, and every output is defined bit
 * for bit, whatever the launch shape and the timing.
 *   - live pairs: pair c is live iff 0 <= src_index[c] < n_s, 0 <= tgt_index[c] < n_t and all six coordinates are finite; in
 *     ascending c the live pairs form the list pair[0 .. live).  live < 3: found = 0, trials = 0;
 *   - hypothesis h = 0 .. max_trials - 1 draws three list positions j_k = min(floor(u(seed, 3 h + k) live), live - 1), u being
 *     fi_mesh_sample's counter hash; a_k is the source point and b_k the target point of pair[j_k], as doubles.  It is invalid
 *     when two of its j_k are equal; when the edge test fails: for (p, q) = (0, 1), (0, 2), (1, 2), with ls the squares of
 *     a_q - a_p and lt those of b_q - b_p summed over ascending axes ((x_0^2 + x_1^2) + x_2^2), min(ls, lt) >= (sim sim)
 *     max(ls, lt) must hold, sim = (double)similarity (no square root; similarity = 0: the test is not made); or when a frame
 *     does not form: u = a_1 - a_0, l_1 = sqrt of its squares summed over ascending axes, e_1 = u / l_1; w = a_2 - a_0,
 *     g = e_1 x w, each component the difference of two products (e_1 w_2 - e_2 w_1, e_2 w_0 - e_0 w_2, e_0 w_1 - e_1 w_0),
 *     l = its length likewise, e_3 = g / l; e_2 = e_3 x e_1; l_1 and l must each be finite and > 0.  The same from b gives
 *     f_1, f_2, f_3.  An invalid hypothesis scores -1;
 *   - transform: R[r][c] = (f_1[r] e_1[c] + f_2[r] e_2[c]) + f_3[r] e_3[c]; c_s = ((a_0 + a_1) + a_2) / 3.0 per component, c_t
 *     likewise from b; t[r] = c_t[r] - ((R[r][0] c_s[0] + R[r][1] c_s[1]) + R[r][2] c_s[2]);
 *   - score: for a live pair (x, y): p_r = ((R[r][0] x_0 + R[r][1] x_1) + R[r][2] x_2) + t[r], d = p - y; the pair is an
 *     inlier iff (d_0^2 + d_1^2) + d_2^2 <= (double)threshold (double)threshold -- a pair exactly at the threshold is in.  The
 *     score is the exact count of inliers among the live pairs; the best hypothesis has the highest score, ties go to the
 *     lowest h; `valid` counts the valid hypotheses scored; no valid hypothesis: found = 0 and the identity;
 *   - batches and the stop: hypotheses are scored in batches of FI_ALIGN_BATCH, the last may be partial.  After every batch,
 *     with T the hypotheses drawn so far (valid or not) and b > 0 the best score: w = b / live, p = (w w) w, q = 1 - p, and
 *     r = q^T by fi_plane_fit's binary exponentiation: stop when r <= 1 - confidence.  confidence = 0 never stops early.
 *     trials reports T;
 *   - result: transform is 4 x 4 row-major, (R t) over (0 0 0 1); inliers[c] is one byte per INPUT pair from the best
 *     hypothesis (0 for a pair that is not live); rms = sqrt(tree_sum((d_0^2 + d_1^2) + d_2^2) / inliers) over the inlier pairs
 *     in ascending c, tree_sum being fi_cluster_measure's; 0 with none.  pairs reports m.  found = 0 leaves the identity,
 *     rms 0 and no inliers.
 * m = 0: found = 0, FI_OK.  FI_ERR_INVALID: NULL opt or out; NULL source, target or indices with a count > 0 that reads
 * them; a negative count; a NaN or negative threshold; similarity outside [0, 1]; confidence outside [0, 1);
 * max_trials outside 1 .. 2^31 - 1; a bad memory kind.  m, n_s or n_t >= 2^31: FI_ERR_UNSUPPORTED.
 * Not offered: 2-D; a least-squares (Kabsch) refit inside the call (fi_points_register is the refit); scale; normal
 * compatibility or distance checks beyond the edge test; fast global registration, 4PCS; slab contexts. */
#define FI_ALIGN_BATCH 16384
typedef struct fi_align_options {
	float              threshold;
	float              similarity;
	long               max_trials;
	double             confidence;
	unsigned long long seed;
} fi_align_options;
typedef struct fi_alignment {
	int    found;
	long   pairs, live, trials, valid, inliers;
	double transform[16];
	double rms;
} fi_alignment;
int fi_align_correspondences(long n_s, const float* source, long n_t, const float* target, long m, const long long* src_index,
                             const long long* tgt_index, const fi_align_options* opt, fi_alignment* out, unsigned char* inliers,
                             int memory);

/* ---- exact distances to a surface; redistancing ------------------------------------------------
 * The contract ("Distances to a surface") is this project's own.  All arithmetic is fp32, one rounding per
 * operation (no FMA contraction):
 *   - primitives: 2-D segments (a, b), 3-D triangles (a, b, c); vertices ndim floats each, in lattice units, interleaved;
 *     indices ndim int32 per primitive, as in fi_mesh.  A primitive with a non-finite vertex coordinate is never nearest; an
 *     index outside [0, num_vertices): FI_ERR_INVALID; ndim other than 2 or 3: FI_ERR_UNSUPPORTED (in 1-D the surface is
 *     points: fi_points_*);
 *   - dot products sum in ascending axis order from the first term;
 *   - segment: ab = b - a; t = dot(q - a, ab) / dot(ab, ab) when dot(ab, ab) > 0, else 0; t clamped to [0, 1];
 *     c = a + t ab per axis;
 *   - triangle: Ericson's ClosestPtPointTriangle (Real-Time Collision Detection 5.1.5), its Voronoi-region tests in its
 *     order, its own expressions (edge AB: a + (d1 / (d1 - d3)) ab; AC: a + (d2 / (d2 - d6)) ac; BC: b + (e / (e + f)) (c - b)
 *     with e = d4 - d3, f = d5 - d6; the face: (a + ab v) + ac w, v = vb r, w = vc r, r = 1 / ((va + vb) + vc)).  A triangle is
 *     degenerate when the branch taken divides by a denominator that is not > 0: the face's (va + vb) + vc, or an edge
 *     region's (Ericson's own code divides 0 / 0 in region AB when a == b, which marching cubes emits at t = 0).  It gives the
 *     nearest of its three edges' segment points (before any clamp), edges ab, bc, ca, the first on ties;
 *   - then c is clamped per axis into the primitive's vertex bounding box (c < lo: lo; c > hi: hi);
 *   - s = 0.0f + (q_0 - c_0)^2 + ... in ascending axes (fi_nearest's s).  A query q: best = min s over the primitives,
 *     distance sqrtf(best), primitive = the smallest index with s == best, closest point = its clamped c.  No usable
 *     primitive or sqrtf(best) > max_distance: +inf, -1, NaN point; a non-finite query: NaN, -1, NaN point;
 *   - results in input order: distances float[n], primitives long long[n] or NULL, closest float[n][ndim] or NULL; they
 *     depend neither on the launch shape nor on timing.
 * n = 0 is fine.  n < 0, NULL required buffers, a NaN or negative max_distance, a bad memory kind: FI_ERR_INVALID; n or the
 * number of primitives >= 2^31: FI_ERR_UNSUPPORTED.  `memory` applies to every buffer of a call; a surface is searched on
 * the device it was created on. */
#define FI_SURFACE_ISO 0  /* the mesh of fi_iso_extract: inside is f < iso */
#define FI_SURFACE_DUAL 1 /* the mesh of fi_dual_contour with central differences: inside is f - iso <= 0 */
int fi_surface_create(fi_surface** out, int ndim, long num_vertices, const float* vertices, long num_primitives,
                      const int* indices, int memory);
/* the same from a mesh of fi_iso_extract* / fi_dual_contour* on the device (no host round trip) */
int fi_surface_from_mesh(fi_surface** out, const fi_mesh* mesh);
int fi_surface_distance(fi_surface* surface, long n, const float* queries, float max_distance, float* distances,
                        long long* primitives, float* closest, int memory);
/* every lattice point of `sizes` (ndim extents >= 1, fewer than 2^31 points, x fastest) as a query: unsigned */
int fi_surface_distance_field(fi_surface* surface, const int* sizes, float max_distance, float* out, long long* primitives,
                              int memory);
int fi_surface_destroy(fi_surface* surface);

/* ---- rays against a surface: hits, crossing counts, containment, signed distances --------------
 * The contract ("Rays"; tests/ray_reference.py restates it in numpy) is this project's own, fixed to the
 * operation (no FMA contraction), over the structure fi_surface_create built:
 *   - a ray is o + t d with t_min <= t <= t_max, both ends closed; d is not normalised and t is in units of d.  A ray with a
 *     non-finite o or d, or d = 0: t = NaN, primitive -1, NaN barycentrics; count 0.  t_min > t_max or a NaN bound:
 *     FI_ERR_INVALID (infinite bounds are fine);
 *   - the projection (Woop, Benthin, Wald: Watertight Ray/Triangle Intersection, JCGT 2013): kz = the axis of the largest
 *     |d|, the lowest on ties; kx, ky the next two in cyclic order, swapped when d[kz] < 0; Sx = d[kx] / d[kz],
 *     Sy = d[ky] / d[kz], Sz = 1 / d[kz] in fp32 (|Sx|, |Sy| <= 1).  Per vertex in fp32: p = v - o,
 *     X = p[kx] - Sx p[kz], Y = p[ky] - Sy p[kz], Z = Sz p[kz];
 *   - the inside test is exact: U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax in fp64 from the fp32 X, Y (exact
 *     products, so exact signs and zeros).  A triangle is a candidate when U, V, W are all >= 0 ("positive") or all <= 0,
 *     and not all zero: a projected triangle of zero area (edge on, coincident vertices) is never hit;
 *   - counted once: a candidate with a zero edge function is hit only if it owns that edge.  Edge B->C belongs to U, C->A to
 *     V, A->B to W; (dx, dy) = end - start in (X, Y), negated when the triangle is not positive; owned when dy > 0, or dy = 0
 *     and dx < 0.  A ray through a shared edge or vertex meets exactly one of the triangles around it on each sheet of the
 *     surface (both or neither at a fold);
 *   - t = fp32(((U Az + V Bz) + W Cz) / ((U + V) + W)), evaluated in fp64, then clamped into [min Z, max Z] of the three
 *     vertices (t < min Z: min Z; t > max Z: max Z); a hit when t_min <= t <= t_max.  Barycentrics: fp32(V / det),
 *     fp32(W / det) with det = (U + V) + W: the weights of b and c;
 *   - 2-D: kz as above, kx the other axis; X = p[kx] - Sx p[kz], Z = Sz p[kz].  A segment (a, b) is crossed when
 *     (Xa > 0) != (Xb > 0) (a shared vertex counts once); in fp64 s = Xa / (Xa - Xb), t = fp32(Za + s (Zb - Za)), clamped
 *     into [min Z, max Z]; the barycentric is fp32(s), the weight of b;
 *   - fi_surface_raycast: t = the smallest hit t in range and the smallest primitive index reaching it; no hit: +inf, -1,
 *     NaN barycentrics.  primitives (long long[n]) and bary (float[n][ndim - 1]) may be NULL;
 *   - fi_surface_count_hits: the hits in range, saturated at limit >= 1 (limit = 1 asks whether anything is in the way);
 *   - fi_surface_contains: inside[i] = the parity (0 / 1) of the unsaturated count of the ray from points[i] along
 *     `direction` (ndim floats on the host whatever `memory`; NULL: +x) over t in [0, +inf).  A mesh that is not closed gives
 *     whatever the parity gives;
 *   - fi_surface_signed_distance(_field): fi_surface_distance(_field)'s values, negated (-0.0f at distance 0, -inf beyond
 *     max_distance) where fi_surface_contains holds along +x; a non-finite query keeps its NaN;
 *   - results in input order; they depend neither on the launch shape nor on timing.
 * Error codes follow fi_surface_distance: n = 0 is fine; n < 0, NULL required buffers, a bad window, limit < 1, a NaN or
 * negative max_distance, a bad memory kind: FI_ERR_INVALID; n >= 2^31: FI_ERR_UNSUPPORTED. */
int fi_surface_raycast(fi_surface* surface, long n, const float* origins, const float* directions, float t_min, float t_max,
                       float* t, long long* primitives, float* bary, int memory);
int fi_surface_count_hits(fi_surface* surface, long n, const float* origins, const float* directions, float t_min, float t_max,
                          int limit, int* counts, int memory);
int fi_surface_contains(fi_surface* surface, long n, const float* points, const float* direction, unsigned char* inside,
                        int memory);
int fi_surface_signed_distance(fi_surface* surface, long n, const float* queries, float max_distance, float* distances,
                               long long* primitives, float* closest, int memory);
int fi_surface_signed_distance_field(fi_surface* surface, const int* sizes, float max_distance, float* out,
                                     long long* primitives, int memory);

/* Redistancing: the signed distance of every lattice point (x fastest) to the field's own iso-surface f = iso -- the mesh of
 * fi_iso_extract (method FI_SURFACE_ISO) or of fi_dual_contour with central differences (FI_SURFACE_DUAL) -- searched as
 * fi_surface_distance_field does.  out = +distance where the point is outside by that producer's rule, -distance (a
 * negation: -0.0f at distance 0) where it is inside; beyond max_distance, or with an empty mesh, +-inf with the sign kept.
 * primitives (NULL or long long[total]) index the mesh returned through `mesh` (NULL, or receives a mesh the caller
 * destroys with fi_mesh_destroy).  A non-finite field value: FI_ERR_INVALID (from the mesh producers); a method other
 * than the two: FI_ERR_INVALID; ndim other than 2 or 3: FI_ERR_UNSUPPORTED.
 * fi_redistance: field = the context's owned values in `memory`, or NULL for the last solution where it lives (an FI_F64
 * solution is rounded to fp32 once, as fi_iso_extract does, and the sign comes from that fp32 field); NULL before the first
 * solve: FI_ERR_STATE.  A slab context (nranks > 1) holds only part of the surface: FI_ERR_UNSUPPORTED; there is no group
 * entry.  `memory` applies to field, out and primitives. */
int fi_redistance(fi_ctx* ctx, const float* field, float iso, int method, float max_distance, float* out, long long* primitives,
                  fi_mesh** mesh, int memory);
/* the same without a context: any whole field, fp32, x fastest */
int fi_redistance_field(const float* field, int ndim, const int* sizes, float iso, int method, float max_distance, float* out,
                        long long* primitives, fi_mesh** mesh, int memory);

/* ---- depth images: oriented points, and a truncated signed distance volume ----------------------------
 * The contract (tests/depth_reference.py is its definition in numpy).  3-D only.  All arithmetic is fp32, one
 * rounding per operation over + - * / sqrt floor min and compares, in the order written here with the parentheses given;
 * nothing is summed by atomics, so a repeated call returns the same bytes.  "valid depth": finite and > 0.
 *
 * A camera: pose = the rows of [R | t], world (lattice coordinates) to camera: c_a = ((R_a0 x + R_a1 y) + R_a2 z) + t_a with
 * R_aj = pose[4 a + j], t_a = pose[4 a + 3].  It looks along +z, image x goes right and y down; pixel (row, col) covers
 * [col, col + 1) x [row, row + 1), its centre is (col + 0.5, row + 0.5); images are row-major, height x width floats.  kind:
 * FI_DEPTH_Z, depth along the optical axis, or FI_DEPTH_RANGE, distance along the pixel's ray.  R is taken as it is given:
 * where it is no rotation, "world point" below is still R^T (c - t).  Cameras are always host structures, whatever `memory`.
 *
 * fi_depth_unproject, a thread per pixel.  For pixel (row, col) with valid depth d:
 *   px = ((col + 0.5) - cx) / fx, py = ((row + 0.5) - cy) / fy;  Z: c = (px d, py d, d);  RANGE: l = sqrt((px px + py py) + 1),
 *   c = ((px / l) d, (py / l) d, (1 / l) d);  e = c - t;  the world point x_j = (R_0j e_0 + R_1j e_1) + R_2j e_2.
 *   A neighbour qualifies when it is in the image, its depth d' is valid and |d' - d| <= max_jump (>= 0; +inf: any).  a = the
 *   world point of the right neighbour minus that of the left one where both qualify; else the one that qualifies against the
 *   pixel's own point (right minus own, or own minus left); b likewise with the lower neighbour minus the upper.  Neither
 *   qualifies in one of the two directions: no normal.  n = (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x), len =
 *   sqrt((n_x n_x + n_y n_y) + n_z n_z), n = n / len.  The ray: v_j = (R_0j c_0 + R_1j c_1) + R_2j c_2, lv = sqrt((v_x v_x +
 *   v_y v_y) + v_z v_z), s = (n_x (v_x / lv) + n_y (v_y / lv)) + n_z (v_z / lv); s > 0: n = -n, s = -s.  incidence = min(-s, 1).
 *   No normal unless len > 0, len finite and incidence > 0.
 * positions float[h w 3], normals float[h w 3], incidence float[h w], valid unsigned char[h w], in pixel order; any may be
 * NULL, not all four.  A pixel without a valid depth: NaN position, zero normal, zero incidence, valid 0 (fi_add_points ignores
 * non-finite points).  A pixel with a position and no normal: valid 1, zero normal, zero incidence.
 *
 * A volume holds tsdf (1 at first) and weight W (0 at first), fp32, for every point of a 3-D lattice, x fastest, on the device
 * that was current at fi_volume_create.  fi_volume_load sets both arrays (to resume a fusion; the values are taken as they
 * are), fi_volume_copy reads them (either output may be NULL).  fi_volume_integrate: the m images lie back to back in depths,
 * image s of height_s x width_s floats; incidences (or NULL) likewise; image_weights (or NULL: all 1) float[m].  Voxel
 * p = (i, j, k), coordinates (float)i, j, k, is updated for image s = 0 .. m - 1 in that order:
 *   1. c = the camera point of p; skip unless c_z > 0;
 *   2. u = fx (c_x / c_z) + cx, v = fy (c_y / c_z) + cy; col = floor(u), row = floor(v); skip if outside the image;
 *   3. d = depth[row, col]; skip unless valid;
 *   4. r = c_z (Z) or sqrt((c_x c_x + c_y c_y) + c_z c_z) (RANGE); e = d - r; skip if e < -truncation (the voxel is hidden:
 *      this cut is on the distance along the ray, before any scaling);
 *   5. q = 1 without incidences; else q = incidence[row, col]: skip unless q >= min_incidence and q is finite;
 *   6. f = min((e q) / truncation, 1): the incidence turns the distance along the ray into one along the normal;
 *   7. w = q image_weight_s; skip unless w > 0;
 *   8. tsdf = (tsdf W + f w) / (W + w), then W = min(W + w, max_weight).
 * The kernel applies FI_DEPTH_CAMERAS images per pass over the volume and takes further passes, in image order, for more; no
 * result depends on that number, nor on the kernel's cull of images a whole run of voxels cannot see.
 *
 * fi_volume_constraints: the voxels with W >= min_weight, W > 0 and |tsdf| < 1, in ascending linear index: positions (float)i,
 * j, k; values tsdf truncation; weights W / max_weight.  Two calls: with all three buffers NULL *n receives the count; else *n
 * holds the room of each given buffer in points on entry (less than the count: FI_ERR_INVALID) and the count on return.
 * fi_add_volume forms those arrays on the device and hands them to the code fi_add_points runs for device buffers, as one
 * batch with values, point weights and no gradient rows: the voxels are data points of the context in every later sense
 * (residuals, robust reweighting, fi_nearest).  With FI_VALUE_NEAREST_NEIGHBOR, whose row reads a gradient for the step from
 * the point to its lattice point, the batch carries zero normals (the step is zero: the row is [1] w = value w); with
 * FI_VALUE_LINEAR_INTERPOLATION it carries none.  The lattice must have the volume's sizes.
 *
 * FI_ERR_INVALID: truncation not > 0 and finite, max_weight not > 0, a NaN min_incidence or min_weight, a NaN or negative
 * max_jump, a kind other than the two, a non-positive image size, a non-finite pose entry, cx or cy, fx or fy not > 0 and
 * finite, a NULL required pointer, a bad memory kind, m < 0, sizes that differ from the lattice's.  m = 0 is fine.
 * FI_ERR_UNSUPPORTED: a 1-D or 2-D lattice, more than 2^31 - 1 voxels, or pixels in one call, a slab context.  `memory` applies
 * to every buffer of a call but the cameras.
 * Not offered: 2-D lattices, bilinear depth lookup, free-space (tsdf = 1) constraints, space carving, sparse or hashed
 * volumes, lens distortion, slab groups.  Colour is fused beside the depth by fi_volume_integrate_colour (below). */
#define FI_DEPTH_Z 0
#define FI_DEPTH_RANGE 1
#define FI_DEPTH_CAMERAS 8
typedef struct fi_camera {
	float pose[12];
	float fx, fy, cx, cy;
	int   width, height, kind;
} fi_camera;
typedef struct fi_volume fi_volume;
int fi_depth_unproject(const fi_camera* camera, const float* depth, float max_jump, float* positions, float* normals, float* incidence,
                       unsigned char* valid, int memory);
int fi_volume_create(fi_volume** out, int ndim, const int* sizes, float truncation, float max_weight);
int fi_volume_destroy(fi_volume* volume);
int fi_volume_load(fi_volume* volume, const float* tsdf, const float* weight, int memory);
int fi_volume_copy(const fi_volume* volume, float* tsdf, float* weight, int memory);
int fi_volume_integrate(fi_volume* volume, long m, const fi_camera* cameras, const float* depths, const float* incidences,
                        const float* image_weights, float min_incidence, int memory);
int fi_volume_constraints(const fi_volume* volume, float min_weight, long* n, float* positions, float* values, float* weights,
                          int memory);
int fi_add_volume(fi_ctx* ctx, const fi_volume* volume, float value_weight, int value_kernel, float min_weight);

/* ---- rays and pinhole images of a lattice field or a depth volume --------------------------------------
 * The contract (tests/march_reference.py is its definition in numpy).  A ray is marched through the trilinear
 * (2-D: bilinear) interpolant of a field to the first crossing of `iso`.  All arithmetic is fp32, one rounding per operation,
 * in the order written here with the parentheses given; min(a, b) is a < b ? a : b and max(a, b) is a > b ? a : b throughout.
 * No atomics, results in input order, nothing depends on the launch: every output is defined bit for bit.
 *
 * The field: fp32, x fastest, ndim 2 or 3, every size >= 2; hi_j = (float)(size_j - 1).  A sample at position p (inside the
 * box): cell c_j = min(floor(p_j), size_j - 2); f(p) = fi_sample's FI_SAMPLE_LINEAR value and g(p) its gradient, the same
 * bits.  The sample is valid when f(p) is finite and, with a weight array (same shape), every corner of the cell has weight > 0
 * and weight >= min_weight.  The unit normal n(p): len = sqrt((g_x g_x + g_y g_y) + g_z g_z) (2-D: sqrt(g_x g_x + g_y g_y)),
 * n = g / len, or zero unless len > 0 and len is finite; it points towards increasing f.  inside(p): f(p) < iso, as
 * fi_iso_extract decides it.
 *
 * A ray o + t d, t_min <= t <= t_max, d not normalised.  len_d = sqrt of the sum of d_j d_j in the order above.  The ray is none
 * (t = NaN, NaN position, zero normal, side 0) where a component of o or d is not finite, or len_d is 0 or not finite.
 *   1. t_enter = -inf, t_exit = +inf; for j = 0 .. ndim - 1: where d_j == 0 the ray is a miss unless 0 <= o_j <= hi_j; else
 *      u = (0 - o_j) / d_j, v = (hi_j - o_j) / d_j, t_enter = max(t_enter, min(u, v)), t_exit = min(t_exit, max(u, v)).
 *      t_a = max(t_enter, t_min), t_b = min(t_exit, t_max).  A miss if t_a > t_b or either is not finite.
 *   2. dt = step / len_d; a miss unless dt > 0 and dt is finite.  Sample k = 0, 1, .. lies at t_k = min(t_a + (float)k dt, t_b);
 *      the last one is the first with t_a + (float)k dt >= t_b, or sample FI_MARCH_MAX_SAMPLES - 1.
 *   3. The sample at t: p_j = o_j + t d_j, then p_j = p_j > 0 ? (p_j > hi_j ? hi_j : p_j) : 0: inside the box
 *      whatever the rounding at the faces did.
 *   4. Two consecutive samples, both valid: a front bracket where the first is outside and the second inside, a back bracket
 *      the other way round.  side: FI_MARCH_FRONT admits front brackets, FI_MARCH_BACK back ones, FI_MARCH_EITHER both.
 *   5. The first admitted bracket (a, b) = (t_k-1, t_k) with values f_a, f_b is refined `refine` times: m = 0.5 (a + b);
 *      the sample at m not valid: stop; inside(m) == inside(a): (a, f_a) = (m, f_m), else (b, f_b) = (m, f_m).  Then
 *      t = a + ((f_a - iso) / (f_a - f_b)) (b - a); the hit's position is the sample position p at t (step 3), its normal
 *      n(p), its side +1 (front) or -1 (back).
 *   6. No admitted bracket, or a miss: t = +inf, NaN position, zero normal, side 0.
 * It can miss two crossings inside one step and anything thinner than `step`.  Outputs t float[n], positions float[n ndim],
 * normals float[n ndim], side signed char[n]; any may be NULL, not all four.
 *
 * An image (3-D only): pixel (row, col) of an fi_camera (above) casts the ray fi_depth_unproject assumes: px, py as there,
 * e_a = 0 - t_a, o_j = (R_0j e_0 + R_1j e_1) + R_2j e_2, d_j = (R_0j px + R_1j py) + R_2j, over t_min = 0, t_max = +inf.
 * depth = t (FI_DEPTH_Z) or t sqrt((px px + py py) + 1) (FI_DEPTH_RANGE); +inf where the ray is a miss or none, which
 * fi_depth_unproject and fi_volume_integrate take as "no depth".  positions float[h w 3], normals float[h w 3], incidence
 * float[h w] as fi_depth_unproject lays them out: s = (n_x (d_x / len_d) + n_y (d_y / len_d)) + n_z (d_z / len_d), q =
 * min(-s, 1); unless q > 0 (a back hit, a zero normal) the normal and the incidence are zero.  A pixel without a hit: NaN
 * position, zero normal, zero incidence.  depth is required, the others may be NULL.
 *
 * fi_raycast_field / fi_render_field: the field of the context's lattice; NULL: its last solution where it lives, an FI_F64
 * one rounded to fp32 once as fi_iso_extract does (FI_ERR_STATE before the first solve).  fi_volume_raycast / fi_volume_render:
 * the field is the volume's tsdf, the weight its W, both read in place; iso 0 is the surface.
 * FI_ERR_INVALID: a non-finite iso, step not > 0 and finite, refine outside 0 .. 16, a side other than the three, a NaN
 * min_weight, t_min > t_max or a NaN bound, a NULL required pointer, every output NULL, a bad memory kind, a bad camera,
 * n < 0.  n = 0 is fine.  FI_ERR_UNSUPPORTED: n, the pixels or the lattice points >= 2^31, ndim = 1, a 2-D field for an image,
 * a slab context.  `memory` applies to every buffer of a call but the camera and a volume's own arrays.
 * Not offered: sphere tracing, empty-space skipping, sorted rays, cubic interpolation, exact per-cell roots, slabs.  The colour
 * image of a volume that carries colour: fi_volume_render_colour (below). */
#define FI_MARCH_FRONT 0
#define FI_MARCH_BACK 1
#define FI_MARCH_EITHER 2
#define FI_MARCH_MAX_SAMPLES 1048576
typedef struct fi_march_options {
	float iso, step, min_weight;
	int   refine, side;
} fi_march_options;
int fi_march_default_options(fi_march_options* options); /* iso 0, step 1, min_weight 0, refine 4, FI_MARCH_FRONT */
int fi_field_raycast(const float* field, const float* weight, int ndim, const int* sizes, const fi_march_options* options, long n,
                     const float* origins, const float* directions, float t_min, float t_max, float* t, float* positions,
                     float* normals, signed char* side, int memory);
int fi_field_render(const float* field, const float* weight, const int* sizes, const fi_march_options* options,
                    const fi_camera* camera, float* depth, float* positions, float* normals, float* incidence, int memory);
int fi_raycast_field(fi_ctx* ctx, const float* field, const fi_march_options* options, long n, const float* origins,
                     const float* directions, float t_min, float t_max, float* t, float* positions, float* normals,
                     signed char* side, int memory);
int fi_render_field(fi_ctx* ctx, const float* field, const fi_march_options* options, const fi_camera* camera, float* depth,
                    float* positions, float* normals, float* incidence, int memory);
int fi_volume_raycast(const fi_volume* volume, const fi_march_options* options, long n, const float* origins,
                      const float* directions, float t_min, float t_max, float* t, float* positions, float* normals,
                      signed char* side, int memory);
int fi_volume_render(const fi_volume* volume, const fi_march_options* options, const fi_camera* camera, float* depth,
                     float* positions, float* normals, float* incidence, int memory);

/* ---- colour in a depth volume --------------------------------------------------------------------------
 * The contract (tests/colour_reference.py is its definition in numpy).  3-D only.  All arithmetic is fp32, one
 * rounding per operation, in the order written here with the parentheses given; min(a, b) is a < b ? a : b.  No atomics:
 * every output is defined bit for bit.
 *
 * A volume gets optional colour state: C = 1 .. 4 channels, fp32, planar (channel k of voxel i at k nvox + i, x fastest), and one
 * colour weight Wc per voxel; channels and Wc are 0 at first.  fi_volume_set_channels allocates and zeroes them (FI_ERR_STATE
 * if the volume has channels already, FI_ERR_INVALID outside 1 .. 4), fi_volume_channels reads C (0: none).
 * fi_volume_colour_load sets float[C nvox] and float[nvox] (the values are taken as they are), fi_volume_colour_copy reads them
 * (either output may be NULL).  fi_volume_load, fi_volume_copy, fi_volume_integrate, fi_volume_constraints, fi_add_volume,
 * fi_volume_raycast and fi_volume_render never touch the colour state.
 *
 * fi_volume_integrate_colour: cameras, depths, incidences, image_weights and min_incidence as fi_volume_integrate takes them;
 * colours holds the images' colours pixel-interleaved, float[h w C] per image, the images back to back like depths.  For
 * image s and voxel p, steps 1 - 8 of fi_volume_integrate run unchanged, with the same e, q, g = (e q) / truncation, f and w:
 * tsdf and W receive the bits fi_volume_integrate gives for the same images.  If the voxel passed step 7, then:
 *   9.  skip the colour unless |g| < band: the voxel lies within band truncation of the surface along the normal (the far
 *       side is cut at step 4 already);
 *   10. skip the colour unless every channel c_k of pixel [row, col] is finite;
 *   11. for k = 0 .. C - 1: a_k = (a_k Wc + c_k w) / (Wc + w); then Wc = min(Wc + w, max_weight).
 * A colour skip never affects the geometry update.  The kernel applies FI_DEPTH_CAMERAS images per pass, further passes in
 * image order for more; no result depends on that number, nor on the cull, nor on whether a pixel's channels are read by one
 * wide load or by C narrow ones.
 *
 * fi_volume_colour_sample, a thread per point, positions float[n 3], hi_j = (float)(size_j - 1).  A point is valid input when
 * it is finite and 0 <= p_j <= hi_j for every j (no clamping).  Cell c_j = min(floor(p_j), size_j - 2), t_j = p_j - c_j,
 * w_0 = 1 - t, w_1 = t per axis.  The corners (a, b, c) of the cell run in ascending a + 2 b + 4 c with omega = (wx_a wy_b) wz_c;
 * a corner counts when its Wc > 0 and Wc >= min_weight.  From S = 0 and N_k = 0, over the counting corners in that order:
 * S = S + omega, N_k = N_k + omega a_k.  colour_k = N_k / S and valid = 1 when S > 0; else (and for a point that is no valid
 * input) colour_k = NaN and valid = 0.  The sums are normalised over the observed corners on purpose: the colour band is thin,
 * and a vertex of the iso-surface sits between a voxel inside it and one outside.  colours float[n C], valid unsigned char[n]
 * or NULL.
 *
 * fi_volume_render_colour: depth, positions, normals and incidence are the bytes fi_volume_render writes for the same
 * options and camera (depth is required, the three may be NULL); colours float[h w C] is fi_volume_colour_sample with
 * colour_min_weight at each pixel's hit position, NaN where there is no hit.
 *
 * fi_volume_colour_constraints: the voxels with Wc > 0 and Wc >= min_weight in ascending linear index: positions (float)i, j,
 * k; colours a_k, interleaved, float[n C]; weights Wc / max_weight.  The two calls of fi_volume_constraints.  Column k of
 * colours is what fi_add_points takes as values (with weights as point weights) to complete channel k by a solve.
 *
 * FI_ERR_STATE: a volume without channels, in every call but the first two.  FI_ERR_INVALID: NULL colours, a band outside
 * (0, 1] or not finite, a NaN min_weight or colour_min_weight, and what fi_volume_integrate and fi_volume_render refuse.
 * m = 0 and n = 0 are fine.  FI_ERR_UNSUPPORTED: sampling or rendering a volume with a size below 2; n >= 2^31.
 * Not offered: 2-D lattices, bilinear image lookup, uint8 storage, colour in pose tracking, colour on fi_mesh handles, slab
 * contexts, gamma or exposure handling, a fused march-and-colour kernel. */
int fi_volume_set_channels(fi_volume* volume, int channels);
int fi_volume_channels(const fi_volume* volume, int* channels);
int fi_volume_colour_load(fi_volume* volume, const float* colour, const float* colour_weight, int memory);
int fi_volume_colour_copy(const fi_volume* volume, float* colour, float* colour_weight, int memory);
int fi_volume_integrate_colour(fi_volume* volume, long m, const fi_camera* cameras, const float* depths, const float* incidences,
                               const float* image_weights, float min_incidence, const float* colours, float band, int memory);
int fi_volume_colour_sample(const fi_volume* volume, float min_weight, long n, const float* positions, float* colours,
                            unsigned char* valid, int memory);
int fi_volume_render_colour(const fi_volume* volume, const fi_march_options* options, const fi_camera* camera,
                            float colour_min_weight, float* depth, float* positions, float* normals, float* incidence, float* colours,
                            int memory);
int fi_volume_colour_constraints(const fi_volume* volume, float min_weight, long* n, float* positions, float* colours, float* weights,
                                 int memory);

#ifdef __cplusplus
}
#endif
#endif /* FI_HIP_H */
