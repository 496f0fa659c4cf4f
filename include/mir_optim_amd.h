/*
 * mir_optim_amd.h -- C ABI of the MI355X-native Levenberg-Marquardt solver.
 *
 * Drop-in boundary for ONE path of libmir/mir-optim: `mir.optim.least_squares`.
 * Part 1 declares exactly the `extern(C)` symbols the reference exports for that path,
 * with ABI-identical structs; each declaration cites the reference interface it replaces
 * (LS = source/mir/optim/least_squares.d, QP = source/mir/optim/boxcqp.d under
 * /root/reference).  Part 2 is additive (device-pointer callbacks, batched residuals,
 * multi-GPU communicator, reusable workspace, statistics); nothing in part 2 exists in the
 * reference.
 *
 * All entry points are re-entrant; no global solver state. Errors never throw or abort:
 * every failure is a negative `status` in the returned struct (LS:132).
 * A process without a usable HIP device gets status = mir_ls_numericError from the solve
 * entry points and a diagnostic on stderr -- there is NO CPU fallback in this library.
 */
#ifndef MIR_OPTIM_AMD_H
#define MIR_OPTIM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ======================================================================================
 * Part 1 -- the reference's extern(C) surface
 * ====================================================================================== */

/* LeastSquaresStatus, LS:20-46 (32-bit enum) */
typedef enum mir_least_squares_status {
    mir_ls_maxIterations = -1,
    mir_ls_furtherImprovement = 0,
    mir_ls_xConverged = 1,
    mir_ls_gConverged = 2,
    mir_ls_fConverged = 3,
    mir_ls_badBounds = -32,
    mir_ls_badGuess = -31,
    mir_ls_badMinStepQuality = -30,
    mir_ls_badGoodStepQuality = -29,
    mir_ls_badStepQuality = -28,
    mir_ls_badLambdaParams = -27,
    mir_ls_numericError = -26
} mir_least_squares_status;

/* BoxQPStatus, QP:18-26 */
typedef enum mir_box_qp_status {
    mir_box_qp_solved = 0,
    mir_box_qp_numericError = 1,
    mir_box_qp_maxIterations = 2
} mir_box_qp_status;

/* BoxQPSettings!T, QP:56-71 */
typedef struct mir_box_qp_settings_d { double relTolerance, absTolerance; uint32_t maxIterations; } mir_box_qp_settings_d;
typedef struct mir_box_qp_settings_s { float relTolerance, absTolerance; uint32_t maxIterations; } mir_box_qp_settings_s;

/* LeastSquaresSettings!double, LS:85-123: 128 bytes, align 8 */
typedef struct mir_least_squares_settings_d {
    uint32_t maxIterations;     /* @0   LS:94  */
    uint32_t maxAge;            /* @4   LS:96  */
    double jacobianEpsilon;     /* @8   LS:98  */
    double absTolerance;        /* @16  LS:100 */
    double relTolerance;        /* @24  LS:102 */
    double gradTolerance;       /* @32  LS:104 */
    double maxGoodResidual;     /* @40  LS:106 */
    double maxStep;             /* @48  LS:108 */
    double maxLambda;           /* @56  LS:110 */
    double minLambda;           /* @64  LS:112 */
    double minStepQuality;      /* @72  LS:114 */
    double goodStepQuality;     /* @80  LS:116 */
    double lambdaIncrease;      /* @88  LS:118 */
    double lambdaDecrease;      /* @96  LS:120 */
    mir_box_qp_settings_d qpSettings;  /* @104 LS:122 */
} mir_least_squares_settings_d;

/* LeastSquaresSettings!float: 68 bytes, align 4 */
typedef struct mir_least_squares_settings_s {
    uint32_t maxIterations, maxAge;
    float jacobianEpsilon, absTolerance, relTolerance, gradTolerance, maxGoodResidual, maxStep,
          maxLambda, minLambda, minStepQuality, goodStepQuality, lambdaIncrease, lambdaDecrease;
    mir_box_qp_settings_s qpSettings;
} mir_least_squares_settings_s;

/* LeastSquaresResult!T, LS:128-143: 32 bytes (double) / 24 bytes (float), returned by hidden pointer */
typedef struct mir_least_squares_result_d {
    int32_t status;             /* LeastSquaresStatus; default numericError (LS:132) */
    uint32_t iterations, fCalls, gCalls;
    double residual;            /* sum of squares, no 1/2, no sqrt (LS:955, LS:1137) */
    double lambda;
} mir_least_squares_result_d;
typedef struct mir_least_squares_result_s {
    int32_t status;
    uint32_t iterations, fCalls, gCalls;
    float residual, lambda;
} mir_least_squares_result_s;

/* mir.ndslice Slice!(T*) 1-D contiguous = { size_t length; T* ptr } (mir-algorithm; LS:713-714) */
typedef struct mir_slice_d { size_t length; double* ptr; } mir_slice_d;
typedef struct mir_slice_s { size_t length; float* ptr; } mir_slice_s;
typedef struct mir_slice_i { size_t length; int32_t* ptr; } mir_slice_i;   /* lapackint = int */

/* LeastSquaresFunctionBetterC / LeastSquaresJacobianBetterC, LS:78-80. J is row-major m x n. */
typedef void (*mir_least_squares_function_d)(void* context, size_t m, size_t n, const double* x, double* y);
typedef void (*mir_least_squares_jacobian_d)(void* context, size_t m, size_t n, const double* x, double* J);
typedef void (*mir_least_squares_function_s)(void* context, size_t m, size_t n, const float* x, float* y);
typedef void (*mir_least_squares_jacobian_s)(void* context, size_t m, size_t n, const float* x, float* J);

/* LeastSquaresTask (an opaque 16-byte D delegate, LS:560-564), LeastSquaresTaskBetterC (LS:567-572)
 * and LeastSquaresThreadManagerBetterC (LS:672-678). The manager must call
 * task(taskContext, totalThreads, threadId, i) once for every i in [0, count). */
typedef struct mir_least_squares_task { void* context; void* function; } mir_least_squares_task;
typedef void (*mir_least_squares_task_function)(mir_least_squares_task task, uint32_t totalThreads,
                                                uint32_t threadId, uint32_t i);
typedef void (*mir_least_squares_thread_manager)(void* context, uint32_t count,
                                                 mir_least_squares_task taskContext,
                                                 mir_least_squares_task_function task);

/* LS:642-646 */
size_t mir_least_squares_work_length(size_t m, size_t n);
/* LS:651-656 */
size_t mir_least_squares_iwork_length(size_t m, size_t n);
/* QP:36-42 */
size_t mir_box_qp_work_length(size_t n);
/* QP:47-50 */
size_t mir_box_qp_iwork_length(size_t n);
/* The same two integer-workspace lengths for builds of the reference with 64-bit `lapackint` (the `*-ilp` dub
 * configurations, dub.sdl:26-80; QP:49 divides by lapackint.sizeof). This library never dereferences iwork, so an ILP64
 * caller only needs lengths that match what its own allocation code expects; every other symbol is layout-identical
 * (Slice!(lapackint*) is {size_t, pointer} for either width). */
size_t mir_box_qp_iwork_length_ilp64(size_t n);
size_t mir_least_squares_iwork_length_ilp64(size_t m, size_t n);
/* LS:666-669 (strings LS:528-557) */
const char* mir_least_squares_status_string(mir_least_squares_status st);
/* LS:761-770 */
void mir_least_squares_init_d(mir_least_squares_settings_d* settings);
void mir_least_squares_init_s(mir_least_squares_settings_s* settings);
/* LS:783-792 */
void mir_least_squares_reset_d(mir_least_squares_settings_d* settings);
void mir_least_squares_reset_s(mir_least_squares_settings_s* settings);

/* LS:705-724. Host-pointer contract of the reference: x/l/u/work/iwork are host memory, f/g/tm
 * are host functions on host memory. The LM arithmetic runs on the GPU; y (and J when g is
 * given) are staged through pinned host buffers. `work`/`iwork` are accepted for ABI
 * compatibility and are not used (device workspace is allocated internally). */
mir_least_squares_result_d mir_optimize_least_squares_d(
    const mir_least_squares_settings_d* settings, size_t m, size_t n,
    double* x, const double* l, const double* u,
    mir_slice_d work, mir_slice_i iwork,
    void* fContext, mir_least_squares_function_d f,
    void* gContext, mir_least_squares_jacobian_d g,
    void* tmContext, mir_least_squares_thread_manager tm);

/* LS:729-748. NOTE: the reference's float entry passes the literal 2 for m (LS:629, a bug);
 * this implementation uses the caller's m. */
mir_least_squares_result_s mir_optimize_least_squares_s(
    const mir_least_squares_settings_s* settings, size_t m, size_t n,
    float* x, const float* l, const float* u,
    mir_slice_s work, mir_slice_i iwork,
    void* fContext, mir_least_squares_function_s f,
    void* gContext, mir_least_squares_jacobian_s g,
    void* tmContext, mir_least_squares_thread_manager tm);

/* ======================================================================================
 * Part 2 -- additive MI355X-native surface (not in the reference)
 * ====================================================================================== */

typedef struct mir_lsq_comm mir_lsq_comm;            /* row-shard communicator */
typedef struct mir_lsq_workspace mir_lsq_workspace;  /* reusable device workspace */

/* Batched residual callback: evaluate p parameter vectors in one sweep over the user's data.
 * X is p x n row-major, Y is p x m row-major (point k's residual vector at Y + k*m); both are
 * DEVICE pointers; work must be enqueued on the options' stream. It is the GPU analogue of the
 * reference's thread manager (LS:184-215): it lets the finite-difference Jacobian evaluate its
 * 2n perturbed points together instead of one at a time. */
typedef void (*mir_lsq_batched_function_d)(void* context, size_t m, size_t n, size_t p, const double* X, double* Y);
typedef void (*mir_lsq_batched_function_s)(void* context, size_t m, size_t n, size_t p, const float* X, float* Y);
enum {
    MIR_LSQ_DEVICE_CALLBACKS = 1u,   /* f/g/fb receive DEVICE pointers and enqueue on `stream` (no host staging) */
    MIR_LSQ_TIME_KERNELS = 2u,       /* bracket the hot kernels with HIP events and fill `stats` */
    MIR_LSQ_FD_BASE_POINT = 4u       /* "my fbRowMajorDiff callback also accepts p = 2n + 1": X then holds the 2n finite-difference
                                        points followed by ONE MORE point (any point: the contract does not say it is their
                                        base). The callback writes the m x n difference panel of the first 2n points to
                                        Y[0 .. m n) exactly as for p = 2n, and the residual VECTOR of the last point to
                                        Y[m n .. m n + m), bit for bit what f writes for that point. With the bit (device
                                        callbacks, no g, a difference panel in one piece, no MIR_LSQ_VARIANT_FD_SEPARATE_FILL)
                                        a solve makes its entry residual f(x0) (LS:953) and the first refresh's panel -- same
                                        x0 -- in one call: a caller whose kernel has each row of its data in hand for the 2n
                                        points saves a whole sweep over the data per solve. Results, fCalls, statistics and the
                                        trace are those of the solve without the bit. One difference a callback can observe:
                                        it is called at the 2n clipped points even when the entry residual already satisfies
                                        fConverged and the reference would stop at LS:974 -- that panel is discarded and its
                                        evaluations are not counted (the rule of discarded ladder trials). Without the bit
                                        p is always 2n. Host callbacks, an analytic Jacobian, the pair-panel and point-major
                                        paths and panels evaluated in pieces keep the separate f(x0) */
};

/* `variant` bits of mir_lsq_gpu_options. 0 = the product path. The first six select LITERAL RESTATEMENTS of the reference's
 * operation order that the parity tests compare the product kernels with (results agree to rounding, several bit for bit);
 * the rest are diagnostics. Read per call, never latched; unknown bits are ignored. (Bit positions are those of earlier
 * releases; the switches of experiments that were measured and retired -- profiles/r03/ab_*.txt -- are gone.) */
enum {
    MIR_LSQ_VARIANT_BROYDEN_REWRITE = 1u << 0,   /* Broyden passes rewrite J every pass (LS:1003-1006 literally) instead of
                                                    the read-only sweep with pending rank-one terms (broyden_lr.h) */
    MIR_LSQ_VARIANT_FD_SEPARATE_FILL = 1u << 1,  /* ignore fbRowMajor / fbRowMajorDiff: point-major panel + column-fill pass
                                                    (LS:1041-1047 as a kernel of its own) + plain J^T J */
    MIR_LSQ_VARIANT_NO_SPECULATION = 1u << 4,    /* one trial per pass instead of the lambda ladder */
    MIR_LSQ_VARIANT_NO_NULL_SKIP = 1u << 5,      /* evaluate f also for trials equal to x bit for bit */
    MIR_LSQ_VARIANT_SOLVE_BOUNDED = 1u << 6,     /* always the solve kernel with the BOXCQP loop compiled in */
    MIR_LSQ_VARIANT_SOLVE_GENERIC = 1u << 10,    /* the any-n solve kernel (solve_big.h) also for n <= 256 */
    MIR_LSQ_VARIANT_SOLVE_ONE_WORKGROUP = 1u << 11, /* n > 256: the any-n solve on ONE workgroup per damping level, without the
                                                    helper workgroups that share its factorisation (solve_coop.h) */
    MIR_LSQ_VARIANT_NO_FD_BASE_POINT = 1u << 14, /* ignore MIR_LSQ_FD_BASE_POINT: f(x0) by a call of its own, p = 2n always
                                                    (A/B runs and tests; bit-identical results either way) */
    MIR_LSQ_VARIANT_FD_WRITE_J = 1u << 15,       /* the fused kernel of the difference panel writes J = D * (1 / twh) on every refresh
                                                    and the Broyden sweeps read J. By default (f64, fbRowMajorDiff, n <= 256, the
                                                    read-only sweep) that write is left out: the unscaled panel stays J0 until the
                                                    next refresh or flush and the sweeps scale what they load; bit-identical
                                                    results either way */
    MIR_LSQ_VARIANT_FD_HOST_COLUMNS = 1u << 13,  /* host-callback finite differences column by column (per-slot staging vectors,
                                                    a strided column write and a stream synchronisation per task, under a
                                                    lock) instead of through the pinned point-major panel */
    MIR_LSQ_VARIANT_NO_PIPELINE = 1u << 22,      /* no FUSED rounds (by default, with device callbacks and n <= 256: the next pass's
                                                    Broyden sweep runs speculatively behind a round's trial residual and carries
                                                    the trial's sum of squares -- one all-reduce for both -- and ONE kernel decides
                                                    the trial, applies the pass's n x n side and solves the next system): every
                                                    round kernel by kernel, decision first; bit-identical results either way */
    MIR_LSQ_VARIANT_DEBUG_HELPERS_ABSENT = 1u << 12, /* diagnostic: the helper workgroups of the any-n solve are NOT launched although
                                                    its kernel expects them -- the first job times out (5 s), the rescue launch
                                                    solves the pass on one workgroup, mir_lsq_stats.coop_timeouts counts it and the
                                                    solve goes on without helpers: the one-workgroup result, no hang (tests) */
    MIR_LSQ_VARIANT_DEBUG_SOLVE = 1u << 7,       /* diagnostic: print phase stamps of the solve kernel (stderr) */
    MIR_LSQ_VARIANT_HOST_PROFILE = 1u << 8,      /* diagnostic: print host wall time per category of runtime call (stderr) */
    MIR_LSQ_VARIANT_LR_CAP_SHIFT = 16            /* bits 16..20 (a field, not a switch): fold the pending Broyden terms into J
                                                    after this many updates (1..16; 0 = 16) */
};

typedef struct mir_lsq_stats {
    uint64_t passes, accepted, rejected, step_guard_rejects;
    uint64_t jacobian_full, jacobian_broyden;
    uint64_t jtj_launches;           /* launches of the fused Broyden + J^T J + J^T y kernel */
    uint64_t jtj_broyden_launches;   /* of those, with the Broyden update fused in */
    double jtj_ms;                   /* sum of event-timed durations of those launches (ms) */
    double jtj_broyden_ms;
    double solve_ms;                 /* n x n damped solve kernel */
    uint64_t solve_launches;
    double fd_ms;                    /* finite-difference refresh, host wall clock: host-callback mode only (device-callback
                                        refreshes are asynchronous: see fd_callback_ms) */
    double total_ms;                 /* whole call, host wall clock */
    uint64_t qp_active_set_passes;   /* passes in which BOXCQP's active-set loop ran */
    uint64_t broyden_lr_columns;     /* sum over the Broyden sweeps of the pending columns each one read (broyden_lr.h) */
    double jtj_fd_ms;                /* of jtj_ms: launches with the finite-difference fill fused in (fbRowMajor) */
    uint64_t jtj_fd_launches;
    uint64_t elided_evaluations;     /* trial evaluations not made because trial == x bit for bit (null steps at the end of
                                        a noisy solve; the callbacks are `pure`, LS:73-80, so f(trial) is already known);
                                        fCalls counts them like the reference does */
    /* row-shard exchanges of this call (counted whenever a communicator is attached, also with one rank):
     * [0] packed [J^T J lower | J^T y] after a full refresh or a resynchronisation: n(n+1)/2 + n elements each
     * [1] sweep vector of a Broyden pass + the sum of squares of the trial residual it was run behind (fused rounds: the ONE
     *     exchange of the round; one-by-one rounds leave that entry unused): 2n + 35 elements each
     * [2] sums of squares of residual vectors that did not ride on a sweep (entry, re-solve rounds, one-by-one rounds) */
    uint64_t allreduce_calls[3];
    uint64_t allreduce_elems[3];
    uint64_t broyden_flushes;        /* times the pending rank-one terms were folded into J */
    uint64_t jtj_resyncs;            /* of those, followed by a recomputation of J^T J / J^T y from the flushed J */
    /* the CALLER's device callbacks, event-timed on the solver's stream (MIR_LSQ_TIME_KERNELS, device-callback mode):
     * finite-difference evaluations (f / fb / fbRowMajor; points = parameter vectors evaluated) and trial evaluations */
    double fd_callback_ms;
    uint64_t fd_callback_calls, fd_callback_points;
    double trial_callback_ms;
    uint64_t trial_callback_calls, trial_callback_points;
    /* ---- everything below: written only when mir_lsq_gpu_options.stats_size says the caller's struct has it ----
     * kernels the LIBRARY launched (the caller's callbacks and memory copies are not counted), by the kind of round they
     * belong to: [0] rounds that start with a full Jacobian refresh (LS:1008-1050), [1] rounds that start with a Broyden
     * update (LS:999-1007), [2] rounds that re-solve with a larger lambda after a rejection (J unchanged); rounds[k] counts
     * the rounds of each kind (a round = update, solve(s), trial residual(s), decision). library_launches also counts what
     * belongs to no round (entry, flushes). */
    uint64_t library_launches;
    uint64_t round_launches[3];
    uint64_t rounds[3];
    /* host-callback finite differences (the reference ABI, LS:1018-1049): wall time of the refreshes (thread manager
     * included), time spent inside the caller's f summed over the manager's threads, columns refreshed */
    double fd_host_wall_ms, fd_host_f_ms;
    uint64_t fd_host_columns;
    double host_f_ms;                /* host-callback mode: wall time inside the caller's f for the entry and trial evaluations */
    uint64_t host_f_calls;
    uint64_t fused_rounds;           /* rounds whose tail was fused (speculative sweep + trial sum, one exchange, one kernel for
                                        decision + n x n side + next solve); fused_passes: of those, the ones whose trial was
                                        accepted with a Broyden pass next -- the pass run ahead was the reference's next pass */
    uint64_t fused_passes;
    uint64_t coop_timeouts;          /* n > 256: ladder entries whose helper workgroups did not answer within 5 s (a GPU shared with
                                        other work) and that were solved again on one workgroup by the rescue launch -- the result
                                        is the MIR_LSQ_VARIANT_SOLVE_ONE_WORKGROUP one (2e-8 from the helpers'), the status is not
                                        touched; after the first one a solve stops asking for helpers */
} mir_lsq_stats;
/* Versioning of mir_lsq_stats: the library writes min(stats_size, sizeof(mir_lsq_stats)) bytes. A caller whose options
 * struct has no stats_size member (struct_size < 96), or leaves it 0, gets the layout of its era: 120 bytes (through
 * qp_active_set_passes) below struct_size 80, 144 (through jtj_fd_launches) below 88, 264 (through trial_callback_points)
 * from 88 on. Changelog: fd_ms is 0 in device-callback mode since the fd_callback_* fields exist (the refresh is only
 * enqueued there); *_callback_calls / *_callback_points are always counted, the *_ms next to them need MIR_LSQ_TIME_KERNELS. */

/* Optional per-pass trace (not in the reference; a parity-pinning aid: tests compare it event by event with the
 * oracle's trace). One record per Jacobian update and per executed loop pass, in the reference's order -- passes
 * evaluated speculatively and then discarded are not recorded.
 *   event 0: Jacobian refreshed in full (LS:1008-1050)   1: Broyden update (LS:999-1007)
 *         2: pass rejected (LS:1125-1130)                3: pass accepted (LS:1132-1139)
 *         4: step-size guard (LS:1101-1106)
 * lambda is the damping the pass solved with; residual the current (event 3: the new) sum of squares;
 * trial_residual ||f(trial)||^2 (0 for events 0, 1, 4); dx_dot = dx.dx of the pass (events 0, 1: of the last
 * accepted step). `count` counts every event even when it exceeds `capacity` (only the first `capacity` are stored). */
typedef struct mir_lsq_trace_record {
    int32_t event;
    uint32_t iterations;
    double lambda, residual, trial_residual, dx_dot;
} mir_lsq_trace_record;
typedef struct mir_lsq_trace {
    mir_lsq_trace_record* records;
    uint64_t capacity;
    uint64_t count;
} mir_lsq_trace;

typedef struct mir_lsq_gpu_options {
    uint32_t struct_size;            /* = sizeof(mir_lsq_gpu_options) */
    uint32_t flags;
    void* stream;                    /* hipStream_t; NULL = a stream owned by the call */
    mir_lsq_comm* comm;              /* NULL = single GPU; else m is this rank's row count */
    mir_lsq_workspace* workspace;    /* NULL = allocate/free per call */
    void* fbContext;
    void* fb;                        /* mir_lsq_batched_function_{d,s} or NULL */
    uint32_t fd_batch;               /* max points per fb call (0 = 2n) */
    uint32_t variant;                /* MIR_LSQ_VARIANT_* bits; 0 = product path */
    mir_lsq_stats* stats;            /* optional out */
    mir_lsq_trace* trace;            /* optional out; read only when struct_size covers it (costs one extra
                                        device-to-host copy per pass) */
    void* fbRowMajor;                /* optional mir_lsq_batched_function_{d,s} that writes Y as m x p ROW-major
                                        (point k's residual of row i at Y[i * p + k]), context fbContext. With it the
                                        finite-difference refresh of f64 problems with n <= 256 needs
                                        no separate column-fill pass: the 2n points are evaluated in one call and the
                                        J^T J kernel forms the Jacobian rows from the (+h, -h) pairs while it writes J.
                                        Read only when struct_size covers it; `fb` is still used for lambda-ladder trials */
    void* fbRowMajorDiff;            /* optional mir_lsq_batched_function_d (f64; n <= 128, n = 192, n = 256), context fbContext: called with the
                                        p = 2n finite-difference points X = [x + h e_0, x - h e_0, x + h e_1, ...] and writes the
                                        m x n ROW-major DIFFERENCE panel D[i * n + j] = f(X_2j)_i - f(X_2j+1)_i -- the caller's
                                        kernel does the reference's copy + axpy(-1) (LS:1041, 1045) on its way out, every one of
                                        the 2n residual vectors is still evaluated. The panel between the caller's kernel and
                                        the library's is then m x n instead of m x 2n: 2 GB less HBM traffic per refresh at
                                        m = 1e6, n = 128 (1 GB not written, 1 GB not read), bitwise the same Jacobian.
                                        Preferred over fbRowMajor when both are given. Read only when struct_size covers it */
    uint32_t stats_size;             /* sizeof(mir_lsq_stats) as the CALLER compiled it: the library never writes past it
                                        (0 or not covered by struct_size: see "Versioning of mir_lsq_stats") */
    uint32_t reserved0;              /* must be 0 */
} mir_lsq_gpu_options;

/* Same algorithm and result contract as mir_optimize_least_squares_{d,s}; x/l/u stay host
 * pointers (n is small); callbacks follow `options->flags`. `options` may be NULL. */
mir_least_squares_result_d mir_optimize_least_squares_gpu_d(
    const mir_least_squares_settings_d* settings, size_t m, size_t n,
    double* x, const double* l, const double* u, const mir_lsq_gpu_options* options,
    void* fContext, mir_least_squares_function_d f,
    void* gContext, mir_least_squares_jacobian_d g,
    void* tmContext, mir_least_squares_thread_manager tm);
mir_least_squares_result_s mir_optimize_least_squares_gpu_s(
    const mir_least_squares_settings_s* settings, size_t m, size_t n,
    float* x, const float* l, const float* u, const mir_lsq_gpu_options* options,
    void* fContext, mir_least_squares_function_s f,
    void* gContext, mir_least_squares_jacobian_s g,
    void* tmContext, mir_least_squares_thread_manager tm);

/* Standalone BOXCQP on the device (the reference's convenience overload QP:85-102 is D-only).
 * P: host row-major n x n, lower triangle meaningful; q,l,u,x host n-vectors. Returns BoxQPStatus
 * (mir_box_qp_numericError also when no device is usable). */
int mir_solve_box_qp_gpu_d(const mir_box_qp_settings_d* settings, size_t n, const double* P,
                           const double* q, const double* l, const double* u, double* x,
                           int unconstrainedSolution, int* iterations);
int mir_solve_box_qp_gpu_s(const mir_box_qp_settings_s* settings, size_t n, const float* P,
                           const float* q, const float* l, const float* u, float* x,
                           int unconstrainedSolution, int* iterations);

/* Batched BOXCQP on the device for small problems: `count` independent solveBoxQP calls (QP:122-379) of the same order
 * n (1 .. 8) in ONE launch, four problems a wavefront (csrc/boxqp_rows.h), instead of a loop over mir_solve_box_qp_gpu_*.
 * All pointers are DEVICE pointers, laid out as mir_lsq_batched_posvx_* takes them: P count x 64 values, problem p at
 * P + 64 p, row-major with row stride 8, the LOWER triangle is read; q and x count x 8; l and u 8 values shared by all
 * problems (bound_stride = 0) or count x 8 (bound_stride = 8). Components >= n are ignored on input and written as 0 in x.
 * status[p]: BoxQPStatus (solved 0; numericError 1: a factorization failed; maxIterations 2, also the all-free exit of the
 * active-set loop); iterations[p] (optional, may be NULL): active-set steps, 0 when the unconstrained minimiser is feasible.
 * settings: relTolerance / absTolerance of the classification, maxIterations (0: 10 n + 100), common to all problems.
 * flags: MIR_LSQ_BOX_QP_UNCONSTRAINED_SOLUTION -- x holds every problem's unconstrained minimiser on entry (the reference's
 * unconstrainedSolution = true, QP:129, 168): the first solve is skipped.
 * The call is enqueued on `stream` (NULL = default stream) and does not synchronise. Returns 0; -1 for bad arguments (a NULL
 * pointer other than iterations, n outside 1 .. 8, bound_stride not 0 or 8, count above 2^30); -5 when the launch failed (no
 * usable device included). count == 0 returns 0 and launches nothing. Callers discover the entry by its name: the version
 * string stays "0.4". */
#define MIR_LSQ_BOX_QP_UNCONSTRAINED_SOLUTION 1u
int mir_lsq_batched_box_qp_s(const mir_box_qp_settings_s* settings, size_t count, size_t n, const float* P, const float* q,
                             const float* l, const float* u, size_t bound_stride, float* x, int* status, int* iterations,
                             unsigned flags, void* stream);
int mir_lsq_batched_box_qp_d(const mir_box_qp_settings_d* settings, size_t count, size_t n, const double* P, const double* q,
                             const double* l, const double* u, size_t bound_stride, double* x, int* status, int* iterations,
                             unsigned flags, void* stream);

/* The same for orders n = 9 .. 16 (csrc/boxqp_rows16.h: four problems a wavefront, one matrix row and one component of every
 * vector per lane of a 16-lane row), in the 16-WIDE layout: P count x 256 values, problem p at P + 256 p, row-major with row
 * stride 16, the LOWER triangle is read; q and x count x 16; l and u 16 values shared by all problems (bound_stride = 0) or
 * count x 16 (bound_stride = 16). Components >= n are ignored on input and written as 0 in x. settings, status, iterations,
 * flags and stream as above. Returns 0; -1 for bad arguments (a NULL pointer other than iterations, n outside 9 .. 16,
 * bound_stride not 0 or 16, count above 2^30); -5 when no device is usable or the launch failed. count == 0 returns 0,
 * launches nothing and needs no device. mir_lsq_batched_box_qp_* keeps rejecting n > 8: the two layouts are separate entries. */
int mir_lsq_batched_box_qp16_s(const mir_box_qp_settings_s* settings, size_t count, size_t n, const float* P, const float* q,
                               const float* l, const float* u, size_t bound_stride, float* x, int* status, int* iterations,
                               unsigned flags, void* stream);
int mir_lsq_batched_box_qp16_d(const mir_box_qp_settings_d* settings, size_t count, size_t n, const double* P, const double* q,
                               const double* l, const double* u, size_t bound_stride, double* x, int* status, int* iterations,
                               unsigned flags, void* stream);

/* The same for orders n = 17 .. 64 (csrc/boxqp_wave.h: one problem a wavefront at n > 32, two at n <= 32; the matrices live
 * in LDS and n is a run-time argument of the kernel), in the DENSE layout: P count x n x n values, problem p at P + n n p,
 * row-major with row stride n, the LOWER triangle is read (what stands above it is never touched); q and x count x n; l and u
 * n values shared by all problems (bound_stride = 0) or count x n (bound_stride = n). settings, status, iterations, flags and
 * stream as above. Returns 0; -1 for bad arguments (a NULL pointer other than iterations, n outside 17 .. 64, bound_stride
 * neither 0 nor n, count above 2^30); -5 when no device is usable or the launch failed. count == 0 returns 0, launches nothing
 * and needs no device. What a problem returns does not depend on its position in the batch. mir_lsq_batched_box_qp16_* keeps
 * rejecting n > 16: the layouts are separate entries. */
int mir_lsq_batched_box_qp64_s(const mir_box_qp_settings_s* settings, size_t count, size_t n, const float* P, const float* q,
                               const float* l, const float* u, size_t bound_stride, float* x, int* status, int* iterations,
                               unsigned flags, void* stream);
int mir_lsq_batched_box_qp64_d(const mir_box_qp_settings_d* settings, size_t count, size_t n, const double* P, const double* q,
                               const double* l, const double* u, size_t bound_stride, double* x, int* status, int* iterations,
                               unsigned flags, void* stream);

/* Batched small fits, ONE WAVEFRONT PER PROBLEM (BASELINE cfg 5): `count` independent problems of the same shape
 * with a built-in residual model r_i = model(t_i; x) - data_i evaluated inside the kernel (no callback):
 *   MIR_LSQ_MODEL_EXP_DECAY   n = 3   p0 exp(-t p1) + p2
 *   MIR_LSQ_MODEL_EXP3_AFFINE n = 8   p0 exp(-t p1) + p2 exp(-t p3) + p4 exp(-t p5) + p6 + p7 t
 * x: count x n (in/out), lower/upper: n (shared; count x n through the _ex entries with MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM), t: m values shared by all problems (t_stride = 0) or count x m
 * (t_stride = m), data: count x m, results: count. All HOST pointers. The LM algorithm, statuses and counters are
 * those of mir_optimize_least_squares_s; problems whose step reaches a finite bound are completed by the general
 * solver (BOXCQP active set) transparently, one problem at a time -- or, with MIR_LSQ_BATCHED_DEVICE_BOUNDS in
 * options->variant, by the wave kernel itself in the same launch. Returns 0, or a negative value: -1 bad arguments, -2 no device, -3 a problem
 * does not fit its workgroup's LDS ((n + 2) m floats <= 160 KB - 512: m <= 4083 at n = 8, 8166 at n = 3), -4 / -5 a failed
 * allocation / launch. */
enum { MIR_LSQ_MODEL_EXP_DECAY = 0, MIR_LSQ_MODEL_EXP3_AFFINE = 1,
       MIR_LSQ_MODEL_EXP_DECAY_PAD8 = 2 };   /* n = 8: p0 exp(-t p1) + p2 + p3 sin 2t + p4 cos 2t + p5 sin 5t + p6 cos 5t + p7 t
                                                (BASELINE cfg 5: the exponential decay padded to n = 8 with terms linear in
                                                their parameters: well conditioned in fp32) */
/* Per-call options of the batched entries (nothing about them is process-wide). NULL = all defaults. */
enum { MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN = 2 };   /* variant bit (launch_batched<Model> with a model that has `grad`): the model's own
                                             derivative instead of finite differences -- the reference's optional g callback:
                                             gCalls counts the refreshes, the default age limit is 3 (least_squares.d:945, 1010) */
enum { MIR_LSQ_BATCHED_NO_LADDER = 1 };   /* variant bit: every damped solve is made for ONE lambda, as the reference's loop does
                                             (boxcqp.d:194 per LS:1080); by default a solve covers lambda and the three values
                                             the rejection rule would give it next (four 16-lane groups of the wave), with
                                             the same steps, bit for bit */
enum { MIR_LSQ_BATCHED_DEVICE_BOUNDS = 4 };   /* variant bit: a damped step that leaves the box is replaced INSIDE the wave kernel by
                                             the solution of the reference's box QP (least_squares.d:1074-1085; boxcqp.d:122-379
                                             with settings->qpSettings), so the one launch finishes every problem: no status
                                             -100 from the kernel entries, nothing left to the general solver in the host
                                             entries. A QP that does not end as solved ends its fit with numericError (-26), as
                                             in the reference. Problems whose steps stay inside the box take the same steps, bit
                                             for bit, with the bit and without it. Not the default: without the bit every entry
                                             does what it always did. launch_batched<Model> answers -1 to it
                                             (launch_batched_bounded<Model> is the header's entry) */
typedef struct mir_lsq_batched_options {
    uint32_t struct_size;     /* = sizeof(mir_lsq_batched_options) */
    uint32_t variant;         /* MIR_LSQ_BATCHED_* bits; 0 = default */
    void* stream;             /* mir_lsq_batched_kernel_s: hipStream_t to enqueue on (NULL = the default stream) */
    float* basis;             /* optional DEVICE buffer for the model's per-row basis table (models with a basis only:
                                 (t_stride ? count : 1) x m x nb floats, 16-byte aligned -- DOUBLES for the _d entries and
                                 any double model: the C type stays float*, basis_bytes counts bytes), owned by the caller and filled by
                                 every call. NULL: the call allocates the table (hipMalloc) and synchronises the stream before
                                 freeing it -- the ONLY case in which mir_lsq_batched_kernel_s synchronises; pass a table to
                                 stay asynchronous (bench.py does) */
    size_t basis_bytes;       /* size of `basis` (the call fails with -1 when it is too small) */
    uint64_t* timing;         /* profiling builds only (-DMIRLSQ_BATCHED_TIMING): DEVICE buffer of 10 cycle counters per
                                 problem, written by the kernel; ignored otherwise */
} mir_lsq_batched_options;

int mir_optimize_least_squares_batched_s(const mir_least_squares_settings_s* settings, size_t count, size_t m, int model,
                                         float* x, const float* lower, const float* upper,
                                         const float* t, size_t t_stride, const float* data,
                                         mir_least_squares_result_s* results, const mir_lsq_batched_options* options);

/* The same wave-per-problem kernel on DEVICE-RESIDENT data (every pointer is a device pointer; `results` receives
 * `count` records in place; enqueued on options->stream, no synchronisation -- see mir_lsq_batched_options.basis for the one
 * exception): what bench.py --config cfg5 times. Problems whose step reaches a finite bound come back with status -100
 * (MIR_LSQ_BATCHED_NEEDS_GENERAL): the host entry above completes those with the general solver, this one leaves that to
 * the caller -- unless options->variant has MIR_LSQ_BATCHED_DEVICE_BOUNDS: then the kernel solves the bounded steps itself
 * and no problem comes back with -100 from either entry. Returns 0 when the launch succeeded. The kernel entry (_s and _d alike) checks its arguments (-1: model id and
 * options, then the pointers and t_stride) before it looks for a device (-2).
 * A caller with a residual model of its own -- the reference takes an arbitrary f, least_squares.d:73-80 -- compiles the
 * same kernel for it from include/mir_optim_amd_batched.hpp (launch_batched<Model>); the three built-in models are
 * instances of that template. */
enum { MIR_LSQ_BATCHED_NEEDS_GENERAL = -100 };
int mir_lsq_batched_kernel_s(const mir_least_squares_settings_s* settings, size_t count, size_t m, int model,
                             float* x, const float* lower, const float* upper,
                             const float* t, size_t t_stride, const float* data,
                             mir_least_squares_result_s* results, const mir_lsq_batched_options* options);

/* The same two entries in DOUBLE (LeastSquaresSettings!double, the reference's main instantiation): the same models (ids and
 * formulas, evaluated in double), contract and return codes as their _s twins; every array is double, the records are the _d
 * ones (32 bytes, written in place by the kernel entry), and a basis table passed in the options holds doubles. A problem
 * needs (n + 2) m doubles of LDS: m <= 2041 at n = 8, 4083 at n = 3. Problems whose step reaches a finite bound are completed
 * by mir_optimize_least_squares_gpu_d in the host entry, and come back with status -100 from the kernel entry; with
 * MIR_LSQ_BATCHED_DEVICE_BOUNDS the kernel finishes them, as in float. */
int mir_optimize_least_squares_batched_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, int model,
                                         double* x, const double* lower, const double* upper,
                                         const double* t, size_t t_stride, const double* data,
                                         mir_least_squares_result_d* results, const mir_lsq_batched_options* options);
int mir_lsq_batched_kernel_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, int model,
                             double* x, const double* lower, const double* upper,
                             const double* t, size_t t_stride, const double* data,
                             mir_least_squares_result_d* results, const mir_lsq_batched_options* options);

/* Per-row WEIGHTS and the COVARIANCE of the fitted parameters on the batched path -- the `sigma` and `pcov` of a curve-fitting
 * interface. The reference takes an arbitrary f (least_squares.d:73-80), so its caller writes (model - data) / sigma_i into f;
 * here the residual is compiled in, and the weights travel in this struct through the _ex entries (mir_lsq_batched_options
 * keeps its size). With weights the residual of row i is
 *     w_i (eval(t_i, x) - data_i),    w_i = 1 / sigma_i for data with per-point uncertainties,
 * everywhere the fit forms a residual or a Jacobian row (finite-difference points are weighted before they are differenced,
 * as through a weighted f). A weight of exactly 0 REMOVES its row: problems of different lengths are padded to a common m and
 * the padding rows given weight 0 (their data must still be finite). Non-finite weights are the caller's error: the
 * host-pointer entry rejects them with -1, the device-pointer entries do not scan (a NaN residual takes the reference's
 * numericError exits).
 * covariance, per problem n x n values row-major, symmetric:
 *     cov = s^2 (J^T J)^-1,  J the (weighted) Jacobian at the returned x, rebuilt as a refresh of the fit builds it,
 *     s^2 = residual / (rows with a nonzero weight - n),  or 1 with MIR_LSQ_BATCHED_ABSOLUTE_SIGMA.
 * Every entry is +inf when J^T J is not positive definite to working precision or the degrees of freedom are <= 0, and NaN
 * when the problem's status is negative (including -100 from the kernel entry: finish the problem, then call
 * mir_lsq_batched_covariance_s / _d).
 * PER-PROBLEM BOUNDS. With MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM in flags, `lower` and `upper` of the call hold count x n values,
 * row k being the box of problem k (host pointers in the mir_optimize_* entries, device pointers in the kernel and covariance
 * entries, as every other pointer); without it they hold n values shared by all problems, as always. Every entry that takes an
 * extras pointer honours the bit (the batched16 entries without _ex too), and an extras that carries only this bit is valid.
 * Each problem is validated against its own row (boundsError, -32, for that problem alone), the -100 problems of the host entry
 * are completed by the general solver with their own rows, and a launch whose rows are all equal gives the bits of the shared
 * launch. The struct keeps its size.
 * FIXED PARAMETERS. A parameter with l_j == u_j in its problem's box is fixed (the `vary = False` of a curve-fit front end). The
 * fit keeps it exactly at that value and minimises over the others. In the covariance its row and column are exactly 0, the
 * other entries are the covariance of the reduced problem, and s^2 = residual / (rows with a nonzero weight - n_free), n_free
 * the number of parameters that are not fixed: the rule of mir_lsq_covariance_gpu_* below. +inf then fills the FREE entries
 * only, when the reduced J^T J is not positive definite or rows - n_free <= 0. A parameter that merely ends on a bound with
 * l_j < u_j is not fixed. */
enum { MIR_LSQ_BATCHED_ABSOLUTE_SIGMA = 1u };
enum { MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM = 2u };
typedef struct mir_lsq_batched_extras {
    uint32_t struct_size;     /* = sizeof(mir_lsq_batched_extras) */
    uint32_t flags;           /* MIR_LSQ_BATCHED_ABSOLUTE_SIGMA, MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM */
    const void* weights;      /* values of the entry's type: m (weight_stride 0) or count x m (weight_stride m); NULL = unweighted */
    size_t weight_stride;     /* 0 or m */
    void* covariance;         /* out: count x n x n values of the entry's type; NULL = not wanted */
} mir_lsq_batched_extras;
/* The two batched entries of each precision with a trailing extras pointer. extras == NULL behaves exactly as the entry
 * without _ex. The pointers in the struct live where the entry's other pointers do (host for
 * mir_optimize_least_squares_batched_ex_*, device for the other two). The argument checks keep their order: -1 for the model
 * id, the options and the extras (struct_size, weight_stride; the host entry's scan for non-finite weights), then the pointers
 * and t_stride, then -2 for the device. The host entry computes the covariance after the general solver has completed the
 * bounded problems, at their final x; the kernel entry computes it on the same stream right after the fit. */
int mir_optimize_least_squares_batched_ex_s(const mir_least_squares_settings_s* settings, size_t count, size_t m, int model,
                                            float* x, const float* lower, const float* upper,
                                            const float* t, size_t t_stride, const float* data,
                                            mir_least_squares_result_s* results, const mir_lsq_batched_options* options,
                                            const mir_lsq_batched_extras* extras);
int mir_optimize_least_squares_batched_ex_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, int model,
                                            double* x, const double* lower, const double* upper,
                                            const double* t, size_t t_stride, const double* data,
                                            mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                                            const mir_lsq_batched_extras* extras);
int mir_lsq_batched_kernel_ex_s(const mir_least_squares_settings_s* settings, size_t count, size_t m, int model,
                                float* x, const float* lower, const float* upper,
                                const float* t, size_t t_stride, const float* data,
                                mir_least_squares_result_s* results, const mir_lsq_batched_options* options,
                                const mir_lsq_batched_extras* extras);
int mir_lsq_batched_kernel_ex_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, int model,
                                double* x, const double* lower, const double* upper,
                                const double* t, size_t t_stride, const double* data,
                                mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                                const mir_lsq_batched_extras* extras);
/* The covariance kernel on its own (device pointers, enqueued on options->stream): for a caller of the kernel entry who has
 * finished its -100 problems itself and written their x and result records back. x and results are read, extras->covariance
 * (required) is written; options->variant selects the analytic Jacobian as in the fit. */
int mir_lsq_batched_covariance_s(const mir_least_squares_settings_s* settings, size_t count, size_t m, int model,
                                 const float* x, const float* lower, const float* upper,
                                 const float* t, size_t t_stride, const float* data,
                                 const mir_least_squares_result_s* results, const mir_lsq_batched_options* options,
                                 const mir_lsq_batched_extras* extras);
int mir_lsq_batched_covariance_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, int model,
                                 const double* x, const double* lower, const double* upper,
                                 const double* t, size_t t_stride, const double* data,
                                 const mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                                 const mir_lsq_batched_extras* extras);

/* Batched fits of models with 9 to 16 PARAMETERS, double precision: one wavefront per problem as above, in a kernel of its own
 * (csrc/batched16_kernel.h): J is held in LDS with a row stride of 16, J^T J is one 16 x 16 tile of the f64 matrix instruction,
 * and the n x n work of a pass runs in the 16-lane-row layout of mir_lsq_batched_box_qp16_d. Finite bounds are handled inside
 * the kernel (the reference's box QP, boxcqp.d:122-379): no problem returns -100 and nothing is left to the general solver; a QP
 * that does not end as solved ends its fit with numericError (-26). Every solve is made for one damping value.
 *   MIR_LSQ_MODEL16_EXP_HARM16     n = 16   p0 exp(-t p1) + p2 + sum_{j = 3 .. 15} p_j h_j(t),  h_j = sin(k w t) for odd j and
 *                                           cos(k w t) for even j, k = (j - 1) / 2 (integer division), w = pi / 2: seven sines
 *                                           and six cosines, a 13-value per-row basis (options->basis: 13 doubles a row)
 *   MIR_LSQ_MODEL16_GAUSS3_AFFINE  n = 11   sum_{k < 3} p_{3k} exp(-((t - p_{3k+1}) / p_{3k+2})^2 / 2) + p9 + p10 t
 * The ids start at 16 and belong to these entries alone: every other batched entry answers -1 to them, and these answer -1 to
 * 0, 1 and 2. Arguments as mir_optimize_least_squares_batched_ex_d (HOST pointers) and mir_lsq_batched_kernel_ex_d (DEVICE
 * pointers, enqueued on options->stream, results in place, no synchronisation except for a basis table the call had to
 * allocate). extras must be NULL or carry neither weights nor covariance: anything else is -1 (weights and covariance have
 * entries of their own, the _ex entries below); its flags may carry MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM (lower / upper: count x n). options->variant: MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN is honoured (-1 for a
 * model without a derivative: GAUSS3_AFFINE); MIR_LSQ_BATCHED_NO_LADDER and MIR_LSQ_BATCHED_DEVICE_BOUNDS are accepted and
 * change nothing. Checks in the usual order: -1 for the model id, the options and the extras, then the pointers and t_stride,
 * then -2 for the device; -3: m = 0 or a problem does not fit its workgroup's LDS ((16 + 2) m + 272 doubles <= 160 KB - 512:
 * m <= 1119); -4 / -5 a failed allocation / launch. A caller's own model of this size: launch_batched16<Model> of
 * include/mir_optim_amd_batched.hpp. */
enum { MIR_LSQ_MODEL16_EXP_HARM16 = 16, MIR_LSQ_MODEL16_GAUSS3_AFFINE = 17 };
int mir_optimize_least_squares_batched16_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, int model,
                                           double* x, const double* lower, const double* upper,
                                           const double* t, size_t t_stride, const double* data,
                                           mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                                           const mir_lsq_batched_extras* extras);
int mir_lsq_batched16_kernel_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, int model,
                               double* x, const double* lower, const double* upper,
                               const double* t, size_t t_stride, const double* data,
                               mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                               const mir_lsq_batched_extras* extras);
/* Per-row WEIGHTS and the COVARIANCE of the fitted parameters for these models: the counterparts of the n <= 8 _ex entries and
 * of mir_lsq_batched_covariance_d, with their meaning of mir_lsq_batched_extras (weights w_i = 1 / sigma_i multiply the residual
 * of their row wherever a residual or a Jacobian row is formed; a weight of exactly 0 removes its row, which is how problems of
 * different lengths share a launch; covariance = s^2 (J^T J)^-1 at the returned x, n x n values a problem, row-major and
 * symmetric, s^2 = residual / (rows with a nonzero weight - n) or 1 with MIR_LSQ_BATCHED_ABSOLUTE_SIGMA; every entry +inf when
 * a pivot of the factorization is not positive or the degrees of freedom are <= 0, NaN when the problem's status is negative).
 * The two entries above keep answering -1 to such extras; these take them, and with extras == NULL they make the fit of the
 * entries above. Arguments, models and return codes are those of the entries above, the order of the checks that of the
 * n <= 8 _ex entries (the host entry answers -1 to a non-finite weight). The weights are read from global memory: the LDS of
 * the fit and m <= 1119 are unchanged; the covariance kernel takes (16 + 1) m + 272 doubles. The kernel entry computes the
 * covariance on the same stream right after the fit; mir_lsq_batched16_covariance_d (DEVICE pointers) computes it alone from
 * the x and the result records (status and residual are read) that a fit left: extras->covariance is required (-1). */
int mir_optimize_least_squares_batched16_ex_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, int model,
                                              double* x, const double* lower, const double* upper,
                                              const double* t, size_t t_stride, const double* data,
                                              mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                                              const mir_lsq_batched_extras* extras);
int mir_lsq_batched16_kernel_ex_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, int model,
                                  double* x, const double* lower, const double* upper,
                                  const double* t, size_t t_stride, const double* data,
                                  mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                                  const mir_lsq_batched_extras* extras);
int mir_lsq_batched16_covariance_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, int model,
                                   const double* x, const double* lower, const double* upper,
                                   const double* t, size_t t_stride, const double* data,
                                   const mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                                   const mir_lsq_batched_extras* extras);
/* Unit-level access to the J^T J stage of that kernel: J count x m x n (row-major, 1 <= n <= 16) and y count x m give, per
 * problem, the 16 x 16 tile J^T J (exactly symmetric; rows and columns >= n are zero) and the 16 values J^T y. DEVICE pointers,
 * enqueued on `stream`. -1 bad arguments, -3 m = 0 or (17 m + 272) doubles above the LDS limit, -2 no device, -5 launch. */
int mir_lsq_batched16_jtj_d(size_t count, size_t m, size_t n, const double* J, const double* y, double* JJ, double* Jy, void* stream);

/* The FITTED CURVE of every problem of a batch on a grid of abscissae of the caller's choice, and its 1-sigma CONFIDENCE BAND --
 * the eval_uncertainty of a curve-fitting interface -- from the x and the covariance a batched fit left on the device:
 *     value[k][i] = eval(tq_i; x_k)                                          always written: a pure function of x
 *     sigma[k][i] = sqrt(max(0, g^T C_k g)),  g = d eval / d x at (tq_i, x_k),  C_k = covariance + k n^2
 * One kernel launch (csrc/batched_predict.h: a wavefront per problem, a query per lane), enqueued on options->stream; every
 * pointer is a DEVICE pointer; no allocation, no synchronisation.
 *   x            count x n                           tq      q values for all problems (tq_stride 0) or count x q (tq_stride q)
 *   covariance   count x n x n, as the covariance entries above write it; required when sigma is given, else not read
 *   value        count x q, required                 sigma   count x q, or NULL: not wanted
 *   lower/upper  both NULL (unbounded, nothing fixed) or both given: n values, or count x n with
 *                MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM in extras->flags
 * g is formed as the covariance kernels form a Jacobian row, without weights and data: the model's derivative with
 * MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN in options->variant (-1 for a model without one), else central differences with
 * settings->jacobianEpsilon, both points clipped to the box. A parameter with l_j == u_j is FIXED: g_j = 0, and row j and column j
 * of the covariance are not read. The sum runs over the free indices in a fixed order of fused multiply-adds: the same input
 * gives the same bits. The conventions of the covariance pass through: when a free diagonal entry C_jj is not finite, every
 * sigma of that problem is that entry (+inf: a degenerate covariance; NaN: a failed fit); all parameters fixed: sigma = 0.
 * extras: NULL, or flags only -- one that carries weights or a covariance pointer is answered -1; other flags are ignored.
 * Returns 0 (also for count == 0 or q == 0, which launch nothing); -1 bad arguments: the model id, implausible options or extras,
 * a missing settings / x / tq / value pointer, one of lower / upper without the other, sigma without covariance, a tq_stride that
 * is neither 0 nor q, count or q >= 2^31 -- all answered before a device is looked for (-2); -5 the launch failed.
 * _s / _d take the MIR_LSQ_MODEL_* ids, mir_lsq_batched16_predict_d the MIR_LSQ_MODEL16_* ids; each answers -1 to the other
 * family's. A caller's own model: launch_batched_predict<Model> of include/mir_optim_amd_batched.hpp. */
int mir_lsq_batched_predict_s(const mir_least_squares_settings_s* settings, size_t count, size_t q, int model, const float* x,
                              const float* lower, const float* upper, const float* tq, size_t tq_stride, const float* covariance,
                              float* value, float* sigma, const mir_lsq_batched_options* options,
                              const mir_lsq_batched_extras* extras);
int mir_lsq_batched_predict_d(const mir_least_squares_settings_d* settings, size_t count, size_t q, int model, const double* x,
                              const double* lower, const double* upper, const double* tq, size_t tq_stride, const double* covariance,
                              double* value, double* sigma, const mir_lsq_batched_options* options,
                              const mir_lsq_batched_extras* extras);
int mir_lsq_batched16_predict_d(const mir_least_squares_settings_d* settings, size_t count, size_t q, int model, const double* x,
                                const double* lower, const double* upper, const double* tq, size_t tq_stride,
                                const double* covariance, double* value, double* sigma, const mir_lsq_batched_options* options,
                                const mir_lsq_batched_extras* extras);

/* Resident-J solver (include/mir_optim_amd_resident.hpp, launch_resident<Model>): the whole loop of least_squares.d:972-1175
 * in ONE cooperative launch for problems whose Jacobian, residuals and per-row data fit the LDS of the chip (BASELINE
 * cfg 2). The residual model is a compile-time type of the caller's, as on the batched path. Options and statistics of
 * that launch; every pointer is a DEVICE pointer. */
enum { MIR_LSQ_RESIDENT_NO_NULL_SKIP = 1u,     /* variant bit: evaluate f also for trials equal to x bit for bit */
       MIR_LSQ_RESIDENT_UNBOUNDED = 2u,         /* variant bit: the caller asserts that every lower / upper entry is infinite
                                                  (the BOXCQP active-set loop is compiled out of workgroup 0's solve) */
       MIR_LSQ_RESIDENT_NO_LOOKAHEAD = 4u,      /* variant bit: every trial gets a round of its own (no sums of squares of the
                                                  next damping levels evaluated along; same results bit for bit, for A/B runs) */
       MIR_LSQ_RESIDENT_DEBUG_DROP_WORKGROUP = 16u, /* diagnostic (tests): the last workgroup leaves before the first round; the
                                                  others' waits are bounded (1 s in this mode, 20 s otherwise) and the launch
                                                  must end with numericError and mir_lsq_resident_stats.abort_code != 0 */
       MIR_LSQ_RESIDENT_ANALYTIC_JACOBIAN = 32u, /* the model's own derivative (Model::jac) instead of finite differences at every
                                                  refresh: the reference's optional g callback (gCalls, age limit 3 by default).
                                                  launch_resident answers -1 for a model without jac */
       MIR_LSQ_RESIDENT_NO_STAMPS = 8u          /* variant bit: mir_lsq_resident_stats carries the counters only, every t_* is 0 (the
                                                  clock reads of workgroup 0 cost a few per cent of a latency-bound fit) */ };
typedef struct mir_lsq_resident_stats {         /* written by the kernel at exit; times in 10 ns ticks of workgroup 0 */
    uint64_t rounds, passes, accepted, rejected, step_guard_rejects, jacobian_full, jacobian_broyden, qp_active_set_passes,
        elided_evaluations;
    uint64_t t_total, t_stage, t_worker, t_group, t_total_wait, t_solver, t_solve_body, t_cmd_wait;
    uint64_t t_w_eval, t_w_fd, t_w_prod;         /* of t_worker: trial residuals, finite-difference refreshes, products + publication */
    uint64_t t_w_mma;                            /* of t_w_prod: the matrix-core loop up to the workgroup's cross-wave hand-over */
    uint64_t lookahead_rejections;               /* rejected passes decided from a sum of squares evaluated along an earlier round */
    uint64_t t_look;                             /* of t_solver: those decisions (own rows + collecting the others' sums) */
    uint64_t t_unpack, t_publish;                /* of t_solver: totals of the 16 groups -> LDS; the next command (constants, stores, drain) */
    uint32_t abort_code, grid, rows, groups;
} mir_lsq_resident_stats;
typedef struct mir_lsq_resident_options {
    uint32_t struct_size;            /* = sizeof(mir_lsq_resident_options) */
    uint32_t variant;                /* MIR_LSQ_RESIDENT_* bits */
    void* stream;                    /* hipStream_t to enqueue on (NULL = the default stream) */
    void* workspace;                 /* optional device scratch of >= resident_workspace_bytes<Model>(m) bytes, owned by the
                                        caller; NULL: the call allocates it and synchronises the stream before freeing it */
    size_t workspace_bytes;
    mir_lsq_trace_record* trace_records;   /* optional per-pass trace (same events as mir_lsq_trace) */
    uint32_t trace_capacity;
    uint32_t max_workgroups;         /* 0 = one workgroup per CU of the device */
    uint32_t* trace_count;           /* events of the solve (also beyond the capacity) */
    mir_lsq_resident_stats* stats;   /* optional */
} mir_lsq_resident_options;

/* Unit-level access to the damped solve of that kernel (?posvx('E','L') with one matrix row per lane; what boxcqp.d:194
 * calls): `count` systems of order n (3 or 8, the orders of the compiled-in models), device pointers; P count x 64 floats,
 * system p at P + 64 p, row-major with row stride 8, the LOWER triangle is read; rhs and x count x 8 floats (components
 * >= n ignored / zero); info[p] = 0 or the order of the leading minor that is not positive (x of that system is zero).
 * Enqueued on `stream`, no synchronisation. */
int mir_lsq_batched_posvx_s(size_t count, size_t n, const float* P, const float* rhs, float* x, int* info, void* stream);
/* the same in double: P count x 64 doubles, rhs and x count x 8 doubles */
int mir_lsq_batched_posvx_d(size_t count, size_t n, const double* P, const double* rhs, double* x, int* info, void* stream);
/* Unit-level access to the 16-row ?posvx('E','L') of mir_lsq_batched_box_qp16_* (csrc/boxqp_rows16.h), four systems a
 * wavefront: `count` systems of order n = 9 .. 16 in the 16-wide layout (P count x 256, row stride 16, the LOWER triangle is
 * read; rhs and x count x 16, components >= n ignored / zero); info[p] as above. Device pointers, enqueued on `stream`, no
 * synchronisation. Returns 0; -1 bad arguments; -2 no device; -5 a failed launch. */
int mir_lsq_batched_posvx16_s(size_t count, size_t n, const float* P, const float* rhs, float* x, int* info, void* stream);
int mir_lsq_batched_posvx16_d(size_t count, size_t n, const double* P, const double* rhs, double* x, int* info, void* stream);
/* Unit-level access to the grid of mir_lsq_batched_box_qp64_*: the same call with a cap on the number of wavefronts launched
 * (max_waves; 0 = the default cap, which is the public entry). With max_waves = 1 one wavefront solves every problem in
 * sequence; the answers are those of any other grid, bit for bit. */
int mir_lsq_batched_box_qp64_waves_s(const mir_box_qp_settings_s* settings, size_t count, size_t n, const float* P, const float* q,
                                     const float* l, const float* u, size_t bound_stride, float* x, int* status, int* iterations,
                                     unsigned flags, void* stream, unsigned max_waves);
int mir_lsq_batched_box_qp64_waves_d(const mir_box_qp_settings_d* settings, size_t count, size_t n, const double* P, const double* q,
                                     const double* l, const double* u, size_t bound_stride, double* x, int* status, int* iterations,
                                     unsigned flags, void* stream, unsigned max_waves);

/* Unit-level access to the hot kernels (parity tests and micro-benchmarks). All pointers are
 * DEVICE pointers; stream may be NULL (default stream; the call synchronises before returning).
 * JJ: n x n row-major, full symmetric on return. broyden != 0 first applies
 *   J += ((y - y_old - J dx) / (dx.dx)) dx^T  (LS:1002-1006) in the same pass. Returns 0 on success. */
int mir_lsq_jtj_d(size_t m, size_t n, double* J, const double* y, const double* y_old, const double* dx,
                  int broyden, double* JJ, double* Jy, void* stream, float* kernel_ms);
int mir_lsq_jtj_s(size_t m, size_t n, float* J, const float* y, const float* y_old, const float* dx,
                  int broyden, float* JJ, float* Jy, void* stream, float* kernel_ms);
/* Finite-difference fill fused into the J^T J kernel (f64; n <= 256; else -6). Yrm: m x 2n
 * row-major, Yrm[i][2j] = f(x + h e_j)_i, Yrm[i][2j+1] = f(x - h e_j)_i; twh[j] = (x_j + h) - (x_j - h) after clipping
 * (0 = collapsed interval: zero column, LS:1046). Writes J (m x n row-major, (Y+ - Y-) * (1 / twh) as LS:1041-1047),
 * JJ = J^T J (full symmetric) and Jy = J^T y. */
int mir_lsq_fd_jtj_d(size_t m, size_t n, const double* Yrm, const double* twh, const double* y, double* J,
                     double* JJ, double* Jy, void* stream, float* kernel_ms);
/* The same from the m x n row-major DIFFERENCE panel D[i][j] = f(x + h e_j)_i - f(x - h e_j)_i (what a fbRowMajorDiff callback
 * writes; f64; n <= 128, n = 192, n = 256, else -6): J = D * (1 / twh) column-wise (zero for twh = 0), JJ, Jy. J may be NULL:
 * the Jacobian rows are formed for J^T J and J^T y only and not written (the solver's default refresh). */
int mir_lsq_fd_diff_jtj_d(size_t m, size_t n, const double* Drm, const double* twh, const double* y, double* J,
                          double* JJ, double* Jy, void* stream, float* kernel_ms);
/* Which kernel those entries and the solver launch (csrc/jtj_plan.h; host code, no device needed): element size 4 / 8, a device
 * of num_cu compute units, op 0 = plain J^T J, 1 = behind the Broyden rewrite (MIR_LSQ_VARIANT_BROYDEN_REWRITE), 2 = the pair
 * panel, 3 = the difference panel, 4 = the difference panel whose caller keeps it as J (mir_lsq_fd_diff_jtj_d with J = NULL);
 * aligned16: J is 16-byte aligned. out = { family (0 none: not covered, 1 k_jtj, 2 k_jtj_fdp, 3 k_jtj_pc32, 4 k_jtj8,
 * 5 k_jtj_fdp8, 6 k_jtj_wide, 7 k_jtj_fdp_nw), 16-column blocks the kernel is compiled for (k_jtj_wide: of n), 1 = the
 * flat producer of k_jtj_fdp, grid x, grid y (tile-pair jobs), dynamic LDS bytes, slabs written, elements per slab, block count
 * the slab reduction is given (0: the tile pairs' own reduction), slab elements a workspace holds }. Returns 0, or -1 (arguments). */
int mir_lsq_jtj_plan(size_t elem_size, size_t m, size_t n, int num_cu, int op, int aligned16, size_t out[10]);

/* Unit-level access to the n x n part of one round of the general solver (csrc/launch_solve.inc: the gradient test LS:1053, the
 * lambda_0 rule LS:1067-1072, P = J^T J + lambda I and the shifted box, solveBoxQP, the rounded step, the step guard, the clamped
 * trial point LS:1087-1110, the predicted reduction LS:1141-1142 and ||trial||_2 LS:1164): ONE launch for the ladder lam[0 .. ks),
 * 1 <= ks <= 8, entry k solving with lam[k]. All pointers are HOST pointers; the call owns its device memory and synchronises.
 * JJ n x n row-major, full symmetric, undamped; Jy, x, lower, upper n values. state_lambda: the lambda of the device-resident
 * state, which entry 0 takes instead of lam[0] with MIR_LSQ_LM_SOLVE_LAMBDA_FROM_STATE (below minLambda: the lambda_0 rule).
 * mode: MIR_LSQ_LM_SOLVE_* bits. FORCE_BOUNDED: the kernel with the BOXCQP loop although every bound is infinite (otherwise the
 * driver's rule: some bound finite); GENERIC: the any-n kernel below n = 257; ONE_WORKGROUP: the any-n kernel without helper
 * workgroups (otherwise the driver's width for n and this device). Fused rounds are not reachable here.
 * Out: rec[0 .. ks): the records the round's decision reads; dx, trial: 8 x n each, rows the kernel did not write hold
 * MIR_LSQ_LM_SOLVE_SENTINEL; *jy_inf: the state's ||J^T y||_inf (written with CHECK_GRAD); JJ, Jy, x, lower, upper: as they are
 * on the device AFTER the launch; info = { kernel class as mir_lsq_lm_solve_class's out[0 .. 2], workgroups per ladder entry
 * (1: no helpers), the first guard band that is not intact or -1, the number of guard bands }. Every device region the kernels
 * are handed (the inputs, dx, trial, the records, the state and each ladder entry's scratch at the workspace's sizes) lies
 * between bands of at least 4 KiB of 0xFF bytes; band b is in front of region b in that order.
 * Returns 0, -1 (arguments), -2 (no device), -3 (allocation / upload), -4 (launch), -5 (synchronisation / download). */
enum { MIR_LSQ_LM_SOLVE_CHECK_GRAD = 1u, MIR_LSQ_LM_SOLVE_LAMBDA_FROM_STATE = 2u, MIR_LSQ_LM_SOLVE_FORCE_BOUNDED = 4u,
       MIR_LSQ_LM_SOLVE_GENERIC = 8u, MIR_LSQ_LM_SOLVE_ONE_WORKGROUP = 16u };
#define MIR_LSQ_LM_SOLVE_SENTINEL (-123456.0)
/* record flags: 1 NaN in the step, 2 NaN in the trial point, 4 step guard LS:1101, 16 gradient test LS:1053 (every other field 0),
 * 32 null step (trial == x bit for bit), 64 the entry's helper workgroups timed out and one workgroup solved it again */
typedef struct { double lambda, new_dx_dot, predicted, trial_xnorm; int32_t qp_status, qp_iterations, flags, reserved; } mir_lsq_lm_solve_record_d;
typedef struct { float  lambda, new_dx_dot, predicted, trial_xnorm; int32_t qp_status, qp_iterations, flags, reserved; } mir_lsq_lm_solve_record_s;
int mir_lsq_lm_solve_d(const mir_least_squares_settings_d* settings, size_t n, double* JJ, double* Jy, double* x, double* lower,
                       double* upper, int ks, const double* lam, double state_lambda, unsigned mode, mir_lsq_lm_solve_record_d* rec,
                       double* dx, double* trial, double* jy_inf, int info[6]);
int mir_lsq_lm_solve_s(const mir_least_squares_settings_s* settings, size_t n, float* JJ, float* Jy, float* x, float* lower,
                       float* upper, int ks, const float* lam, float state_lambda, unsigned mode, mir_lsq_lm_solve_record_s* rec,
                       float* dx, float* trial, float* jy_inf, int info[6]);
/* Which kernel launch_lm_solve runs (host code, no device needed): element size 4 / 8; bounded: some bound finite (or forced);
 * generic: the any-n kernel asked for; diagnostic: the phase-stamp buffer is attached. out = { 0 one wave per ladder entry
 * (k_lm_solve_wave: f64, n <= 16) / 1 one 256-thread workgroup (k_lm_solve) / 2 the any-n kernel (k_lm_solve_big), the 16-row LDS
 * blocks a side the workgroup kernel is compiled for (1, 2, 4, 8; 0: factor in global memory), 1 = the instance with the BOXCQP
 * loop (always 1 for the any-n kernel) }. Returns 0, or -1 (arguments). */
int mir_lsq_lm_solve_class(size_t elem_size, size_t n, int bounded, int generic, int diagnostic, int out[3]);

/* Unit-level access to the read-only Broyden sweep (the default path's Broyden pass for n <= 512). J (m x n row-major), U (16
 * columns of length m), D (16 x n), dx (n), dx_dot (one value: dx.dx), y (count vectors of length m, m apart; vector 0 is the
 * new residual), y_old (m), JJ (n x n), Jy (n) are DEVICE pointers of the caller's; partials, reduced, sums, jy_inf are HOST
 * pointers. The call owns the rest of its device memory, keeps no state and synchronises before it returns.
 * mir_lsq_lr_pass_*: the launches of one pass with k pending terms (0 <= k < 16), in the solver's order and on the solver's
 * workgroup count nblk = mir_lsq_lr_blocks(m, 0): the sweep (writes column k of U and nblk partial vectors of
 * len = 2 n + 35 values [ v0 (n) | g0 (n) | w (16) | h (16) | uu | uy | yy ]), their fixed-order sum (`reduced`, len values), the
 * n x n side (JJ += v dx^T + dx v^T + uu dx dx^T, Jy, row k of D = dx, the state's ||J^T y||_inf -> *jy_inf); then the two-stage
 * sums of squares of the `count` vectors at y (1 <= count <= 8) -> sums, whose entry 0 has the bits of reduced[len - 1].
 * spec != NULL: the speculative sweep of a fused round on that record with the two tolerances -- a record after which no Broyden
 * pass can follow makes the sweep write ||y||^2 and zeros only; the n x n side is NOT run in this mode (it lives in the solve
 * kernel), JJ, Jy, D and *jy_inf stay as they were.
 * info = { column-pair chunks a lane (1, 2, 4, 8, 16), 1 = vector loads, nblk, the first guard band that is not intact or -1
 * (band b in front of: 0 the partials, 1 the reduced vector, 2 the stage-1 partials of the sums, 3 the sums, 4 the state, 5 the
 * record; 6 behind it), the number of bands, 1: a state field other than jy_inf was written | 2: the record changed }.
 * mir_lsq_lr_flush_*: J += u_0 dx_0^T + ... + u_{k-1} dx_{k-1}^T in place (1 <= k <= 16); info = { chunks, vector loads }.
 * Returns 0, -1 (arguments), -2 (no device), -3 (allocation / upload), -4 (launch), -5 (synchronisation / download). */
int mir_lsq_lr_pass_d(size_t m, size_t n, int k, const double* J, double* U, double* D, const double* dx, const double* dx_dot,
                      const double* y, int count, const double* y_old, double* JJ, double* Jy, const mir_lsq_lm_solve_record_d* spec,
                      double absTolerance, double relTolerance, double* partials, double* reduced, double* sums, double* jy_inf,
                      int info[6]);
int mir_lsq_lr_pass_s(size_t m, size_t n, int k, const float* J, float* U, float* D, const float* dx, const float* dx_dot,
                      const float* y, int count, const float* y_old, float* JJ, float* Jy, const mir_lsq_lm_solve_record_s* spec,
                      float absTolerance, float relTolerance, float* partials, float* reduced, float* sums, float* jy_inf,
                      int info[6]);
int mir_lsq_lr_flush_d(size_t m, size_t n, int k, double* J, const double* U, const double* D, int info[2]);
int mir_lsq_lr_flush_s(size_t m, size_t n, int k, float* J, const float* U, const float* D, int info[2]);
/* The same pass and flush when the refresh did not write J (the default with a fbRowMajorDiff callback; f64, n <= 256): P is the
 * unscaled m x n difference panel (what mir_lsq_fd_diff_jtj_d reads) and twh its n interval widths, both DEVICE pointers. The
 * sweep scales what it loads, d * (1 / twh) or 0 for twh = 0: every output has the bits of mir_lsq_lr_pass_d on the J that
 * mir_lsq_fd_diff_jtj_d writes from P and twh. The flush writes J = scale(P) + the k terms and leaves P as it is. The instance is
 * mir_lsq_lr_class(8, n, P -- for the flush P and J -- on the grid of two elements). */
int mir_lsq_lr_pass_scaled_d(size_t m, size_t n, int k, const double* P, const double* twh, double* U, double* D, const double* dx,
                             const double* dx_dot, const double* y, int count, const double* y_old, double* JJ, double* Jy,
                             const mir_lsq_lm_solve_record_d* spec, double absTolerance, double relTolerance, double* partials,
                             double* reduced, double* sums, double* jy_inf, int info[6]);
int mir_lsq_lr_flush_scaled_d(size_t m, size_t n, int k, double* J, const double* P, const double* twh, const double* U, const double* D,
                              int info[2]);
/* The kernel instance the sweep and the flush run (host code, no device needed): element size 4 / 8, n <= 512, aligned: J lies on
 * the grid of two elements. out = { chunks a lane, 1 = vector loads (even n and aligned) }. Returns 0, or -1 (arguments). */
int mir_lsq_lr_class(size_t elem_size, size_t n, int aligned, int out[2]);
/* Workgroups of the sweep for m rows on num_cu compute units (num_cu <= 0: the current device's). Returns the count (1 .. 1024),
 * -1 (arguments) or -2 (no device). */
int mir_lsq_lr_blocks(size_t m, int num_cu);

/* Unit-level access to the decision and bookkeeping kernels of the general solver's round (csrc/misc_kernels.h). All pointers are
 * HOST pointers; each call owns its device memory, keeps no state and synchronises. Every region a kernel is handed lies in one
 * allocation preset to 0xFF bytes with at least 4 KiB of them in front of it and behind it (as mir_lsq_lm_solve_*'s); "guard" below is
 * the first band that is not intact, or -1, "bands" their number. Return values as mir_lsq_lm_solve_*'s.
 * mir_lsq_lm_state_*: the device-resident scalars of the LM loop (csrc/solve_types.h, LmState), field for field.
 * mir_lsq_decide_*: ONE launch of the decision kernel (LS:1080-1161 over a ladder of ks trials, 1 <= ks <= 8) with the solver's
 * geometry. In and out (each comes back as it is on the device after the launch): state; rec[ks]; sums[ks] (the trials' sums of
 * squares); x[n]; trial, dx_chain (ks x n); dx_acc[n]; partials (ks x pstride; nparts > 0: sums[k] is first formed from the nparts
 * stage-1 partials at partials + k pstride; nparts = 0: partials may be NULL). mode: MIR_LSQ_DECIDE_* bits; with MIRROR the state
 * and the accepted point are also published to pinned, device-mapped host memory preset to 0xFF (host_state, host_x[n] return
 * it), without it the kernel is given no mirror and both come back as 0xFF bytes. info = { guard, bands } (the mirror's bands
 * follow the device's: state, x[n]).
 * mir_lsq_fd_points_*: ONE launch of the finite-difference points (LS:1027-1031) for x, lower, upper (n values each, n <= 4096)
 * and the step eps: X ((2 n + with_base) x n: row 2 j = x with x_j + eps clipped to upper_j, row 2 j + 1 = x with x_j - eps clipped
 * to lower_j, with_base: row 2 n = x), twh[n] the widths the device computed, twh_host[n] the solver's host copy of them.
 * mir_lsq_fd_fill_*: ONE launch of the column fill (LS:1037-1046) for the panel of columns [j0, j0 + pc): Y 2 pc rows of m values,
 * ldy >= m apart (the two points of column j0 + c in rows 2 c, 2 c + 1), twh[n], J (m x n row-major, in and out). col != 0 (pc = 1):
 * the single-column kernel of host-callback mode on rows 0 and 1 of Y with twh[j0].
 * mir_lsq_entry_state_*: the entry of a solve (LS:953-971): the two-stage sum of squares of v[0 .. m) on mir_lsq_sumsq_blocks(m)
 * workgroups (partials[nb], *sum), the initial state from it (state; host_state its pinned mirror, sequence number seq); then
 * the same stage 1 on a grid of nb x 2 over v[0 .. m) and v[m .. 2m) (partials2: 2 x nb) and stage 2 on two workgroups (sums2[2]);
 * then the forced refresh's mu = 1 (LS:984-989) on the image st2. info = { nb, guard, bands }.
 * mir_lsq_unpack_grad_*: ONE launch that expands packed = [ lower triangle of J^T J by rows | J^T y ] (n (n + 1) / 2 + n values,
 * n <= 4096) into JJ (n x n), Jy and the state's jy_inf = ||J^T y||_inf (LS:1053); state is an image in and out. */
typedef struct {
    double lambda, mu, residual, trial_residual, dx_dot, new_dx_dot, predicted, trial_xnorm, jy_inf, improvement, rho, pad0;
    int32_t qp_status, qp_iterations, flags, decision; uint32_t iterations; int32_t accepted_k;
    uint32_t consumed, fcalls, rejects, guards, qp_active, null_tail, seq, coop_rescued; int32_t spec_ok;
} mir_lsq_lm_state_d;
typedef struct {
    float lambda, mu, residual, trial_residual, dx_dot, new_dx_dot, predicted, trial_xnorm, jy_inf, improvement, rho, pad0;
    int32_t qp_status, qp_iterations, flags, decision; uint32_t iterations; int32_t accepted_k;
    uint32_t consumed, fcalls, rejects, guards, qp_active, null_tail, seq, coop_rescued; int32_t spec_ok;
} mir_lsq_lm_state_s;
enum { MIR_LSQ_DECIDE_CHECK_GRAD = 1u, MIR_LSQ_DECIDE_LAMBDA_FROM_STATE = 2u, MIR_LSQ_DECIDE_SPEC_STATIC = 4u, MIR_LSQ_DECIDE_MIRROR = 8u };
int mir_lsq_decide_d(const mir_least_squares_settings_d* settings, size_t n, int ks, unsigned mode, uint32_t maxIterations, uint32_t seq,
                     mir_lsq_lm_state_d* state, mir_lsq_lm_solve_record_d* rec, double* sums, double* x, double* trial, double* dx_chain,
                     double* dx_acc, double* partials, int nparts, int pstride, mir_lsq_lm_state_d* host_state, double* host_x, int info[2]);
int mir_lsq_decide_s(const mir_least_squares_settings_s* settings, size_t n, int ks, unsigned mode, uint32_t maxIterations, uint32_t seq,
                     mir_lsq_lm_state_s* state, mir_lsq_lm_solve_record_s* rec, float* sums, float* x, float* trial, float* dx_chain,
                     float* dx_acc, float* partials, int nparts, int pstride, mir_lsq_lm_state_s* host_state, float* host_x, int info[2]);
int mir_lsq_fd_points_d(size_t n, const double* x, const double* lower, const double* upper, double eps, int with_base, double* X,
                        double* twh, double* twh_host, int info[2]);
int mir_lsq_fd_points_s(size_t n, const float* x, const float* lower, const float* upper, float eps, int with_base, float* X,
                        float* twh, float* twh_host, int info[2]);
int mir_lsq_fd_fill_d(size_t m, size_t n, size_t ldy, int j0, int pc, const double* Y, const double* twh, double* J, int col, int info[2]);
int mir_lsq_fd_fill_s(size_t m, size_t n, size_t ldy, int j0, int pc, const float* Y, const float* twh, float* J, int col, int info[2]);
int mir_lsq_entry_state_d(size_t m, const double* v, uint32_t seq, double* partials, double* sum, mir_lsq_lm_state_d* state,
                          mir_lsq_lm_state_d* host_state, double* partials2, double* sums2, mir_lsq_lm_state_d* st2, int info[3]);
int mir_lsq_entry_state_s(size_t m, const float* v, uint32_t seq, float* partials, float* sum, mir_lsq_lm_state_s* state,
                          mir_lsq_lm_state_s* host_state, float* partials2, float* sums2, mir_lsq_lm_state_s* st2, int info[3]);
/* workgroups of the entry residual's sum of squares for m rows (host code); -1: m == 0 */
int mir_lsq_sumsq_blocks(size_t m);
int mir_lsq_unpack_grad_d(size_t n, const double* packed, mir_lsq_lm_state_d* state, double* JJ, double* Jy, int info[2]);
int mir_lsq_unpack_grad_s(size_t n, const float* packed, mir_lsq_lm_state_s* state, float* JJ, float* Jy, int info[2]);

/* Covariance of the fitted parameters of the general solver: cov = s^2 inv(J^T J) at x (usually the x a solve returned), from
 * ONE full Jacobian refresh made exactly as a refresh of the solve makes it (g if given, else finite differences through the
 * same callbacks, options->fb / fbRowMajor / fbRowMajorDiff, fd_batch and clipping of x +- jacobianEpsilon to [l, u]), the J^T J
 * kernel of the solve (all-reduced over options->comm) and an SPD inverse on the device; nothing of the LM loop runs and x is not
 * written. s^2 = ||f(x)||^2 / (M - n_free): M the rows of all ranks, n_free the parameters with l_j < u_j; with
 * MIR_LSQ_COVARIANCE_ABSOLUTE_SIGMA s^2 = 1; with M - n_free <= 0 every free entry is +inf. A parameter with l_j == u_j is
 * fixed: its row and column are 0. A parameter ON a bound with l_j < u_j is not fixed (its difference is one-sided or narrower).
 * options->workspace, stream, comm, stats (the refresh and callbacks are counted in the existing fields) are honoured, trace is
 * ignored; the n x n scratch comes from the workspace, a workspace stays usable by later solves.
 * cov: HOST, n x n row-major. Returns 0 (cov written; *info as the inverse's: nonzero -> +inf at the free entries),
 * mir_ls_badGuess (-31: x NULL or not finite, m == 0, n == 0), mir_ls_badBounds (-32), the status of a bad setting, -1 (settings,
 * l, u, cov or f NULL), or mir_ls_numericError (-26) when no device is usable or a launch failed. These are answered before a
 * device is touched, except the last. residual_out (optional): ||f(x)||^2; info (optional). n <= 20480 (double), 40960 (float). */
enum { MIR_LSQ_COVARIANCE_ABSOLUTE_SIGMA = 1u };
int mir_lsq_covariance_gpu_d(const mir_least_squares_settings_d* settings, size_t m, size_t n,
    const double* x, const double* l, const double* u, const mir_lsq_gpu_options* options,
    void* fContext, mir_least_squares_function_d f, void* gContext, mir_least_squares_jacobian_d g,
    void* tmContext, mir_least_squares_thread_manager tm,
    uint32_t flags, double* cov, double* residual_out, int* info);
int mir_lsq_covariance_gpu_s(const mir_least_squares_settings_s* settings, size_t m, size_t n,
    const float* x, const float* l, const float* u, const mir_lsq_gpu_options* options,
    void* fContext, mir_least_squares_function_s f, void* gContext, mir_least_squares_jacobian_s g,
    void* tmContext, mir_least_squares_thread_manager tm,
    uint32_t flags, float* cov, float* residual_out, int* info);
/* Unit-level access to the inverse (csrc/spd_inverse.h): X = inv(P), equilibrated as ?posvx('E') and factored by a lower
 * Cholesky. DEVICE pointers; P n x n row-major (lower triangle read); fixed: n bytes or NULL -- a nonzero byte takes that index
 * out of the system (its row and column of P are not read and are 0 in X); X n x n, symmetric to the bit; info: device int, 0 or
 * the 1-based order, among the free indices, of the first leading minor that is not positive (a NaN included): every free entry
 * of X is then +inf. Deterministic. The call allocates its scratch, enqueues on `stream` (NULL = default stream) and
 * synchronises that stream before it returns, as mir_lsq_jtj_*. Returns 0, -1 (n == 0, n too large, NULL pointer), -2 (no
 * device), -3 (allocation), -4 (launch), -5 (synchronisation). */
int mir_lsq_spd_inverse_d(size_t n, const double* P, const unsigned char* fixed, double* X, int* info, void* stream);
int mir_lsq_spd_inverse_s(size_t n, const float*  P, const unsigned char* fixed, float*  X, int* info, void* stream);
/* The same with caller-owned DEVICE scratch of mir_lsq_spd_inverse_work_bytes(n, element size) bytes: two launches enqueued
 * on `stream`, no allocation and no synchronisation (what a caller times, or runs behind its own kernels). */
size_t mir_lsq_spd_inverse_work_bytes(size_t n, size_t elem_size);
int mir_lsq_spd_inverse_work_d(size_t n, const double* P, const unsigned char* fixed, double* X, int* info, void* work,
                               size_t work_bytes, void* stream);
int mir_lsq_spd_inverse_work_s(size_t n, const float* P, const unsigned char* fixed, float* X, int* info, void* work,
                               size_t work_bytes, void* stream);

/* Workspace: device buffers for one (m, n, element size) problem, reusable across calls. */
mir_lsq_workspace* mir_lsq_workspace_create(size_t m, size_t n, size_t elem_size);
void mir_lsq_workspace_destroy(mir_lsq_workspace* ws);

/* Row-shard communicators: one fused sum-all-reduce of the packed
 * [J^T J lower | J^T y] buffer per Jacobian-changing pass, one 1-scalar all-reduce per trial step. */
int mir_lsq_rccl_unique_id(void* out_128_bytes);                       /* ncclGetUniqueId */
mir_lsq_comm* mir_lsq_comm_create_rccl(int nranks, int rank, const void* unique_id_128_bytes);
/* callback communicator: `allreduce(ctx, device_buf, count_of_doubles, stream)` must sum `buf` over
 * ranks in place, ordered after prior work on `stream` (used with gloo in the tests). */
typedef void (*mir_lsq_allreduce_fn)(void* ctx, double* device_buf, size_t count, void* stream);
mir_lsq_comm* mir_lsq_comm_create_callback(int nranks, int rank, mir_lsq_allreduce_fn fn, void* ctx);
/* In-process group: `nranks` solver instances inside ONE process -- one host thread each, on the same device (R logical
 * shards on one GPU: the single-device emulation of SURVEY.md section 7 step 7) or on different devices (one process
 * driving several GPUs without RCCL). An all-reduce copies each rank's buffer to pinned host memory, the ranks meet at a
 * barrier, every rank sums the nranks contributions in rank order (bitwise identical totals on all ranks) and copies the
 * total back. out_comms receives nranks handles (rank r at out_comms[r]); destroy each with mir_lsq_comm_destroy -- in any
 * order and from any thread, also while other ranks are still solving: the shared slots live until the last handle goes.
 * A rank that waits longer than 120 s at the barrier gives up (the solve then returns numericError). Returns 0. */
int mir_lsq_comm_create_local_group(int nranks, mir_lsq_comm** out_comms);
void mir_lsq_comm_destroy(mir_lsq_comm* comm);
/* Record / replay of a rank's exchanges (a measurement tool: bench.py --replay-ranks). A rank of an
 * in-process group can RECORD the totals of all its all-reduces (as doubles, concatenated in call order) into a caller-owned
 * host buffer: mir_lsq_comm_record(comm, buf, capacity_in_doubles) before the solve, mir_lsq_comm_recorded(comm) after it
 * (the doubles written; (size_t)-1 after an overflow). A REPLAY communicator then lets ONE rank run alone on exactly the global
 * trajectory: every all-reduce REPLACES the buffer by the next recorded total (a stream-ordered device copy; the rank's own
 * contribution is computed and discarded) and, when `inner` is given, passes it through inner's all-reduce as well (a
 * one-rank RCCL communicator: the launch cost of the real collective). mir_lsq_comm_replay_rewind restarts the tape for the
 * next solve. f64 problems only. The replay handle does not own `inner`. */
int mir_lsq_comm_record(mir_lsq_comm* comm, double* host_buf, size_t capacity);
size_t mir_lsq_comm_recorded(const mir_lsq_comm* comm);
mir_lsq_comm* mir_lsq_comm_create_replay(int nranks, int rank, const double* totals_host, size_t len, mir_lsq_comm* inner);
int mir_lsq_comm_replay_rewind(mir_lsq_comm* comm);
/* A MODEL of the collectives' latency for the replay tool: every replayed exchange first holds the stream for `microseconds`
 * (one idle wave), so that a one-GPU replay of a rank charges each all-reduce what an N-rank RCCL call is ASSUMED to cost --
 * bench.py --replay-ranks R --replay-latency-us L prints the solve time as a function of that assumption. 0 = off. */
int mir_lsq_comm_replay_set_delay(mir_lsq_comm* comm, unsigned microseconds);
/* ranks of the communicator as its transport reports them (RCCL: ncclCommCount); -1 on error */
int mir_lsq_comm_ranks(const mir_lsq_comm* comm);
/* One line about the transport, for logs: "rccl path=<shared object ncclAllReduce was bound from> version=<ncclGetVersion>
 * preloaded=<1: the host program had it mapped already> ranks=<ncclCommCount> rank=<r>", or "callback ..." / "local-group ...".
 * snprintf semantics (returns the length it needs). bench.py puts it into its JSON line: the library binds an RCCL the
 * host program has already loaded (PyTorch's) in preference to /opt/rocm's, and a version skew should be visible. */
int mir_lsq_comm_describe(const mir_lsq_comm* comm, char* buf, size_t len);
/* Sum `count` doubles (floats) of the DEVICE buffer `buf` over the communicator's ranks, in place, ordered on `stream` -- the
 * collective the solver issues for the three exchanges of a pass (least_squares.d:1052, 1065, 1115), exposed so that a caller
 * can check a communicator before the first solve (bench.py does). Returns 0 on success. */
int mir_lsq_comm_allreduce_d(mir_lsq_comm* comm, double* buf, size_t count, void* stream);
int mir_lsq_comm_allreduce_s(mir_lsq_comm* comm, float* buf, size_t count, void* stream);

/* Small device utilities for language bindings that have no HIP runtime of their own. */
int mir_lsq_device_count(void);
void* mir_lsq_device_malloc(size_t bytes);
void mir_lsq_device_free(void* p);
int mir_lsq_memcpy_h2d(void* dst_device, const void* src_host, size_t bytes, void* stream);
int mir_lsq_memcpy_d2h(void* dst_host, const void* src_device, size_t bytes, void* stream);
int mir_lsq_memcpy_d2d(void* dst_device, const void* src_device, size_t bytes, void* stream);   /* asynchronous */

/* Self-test of the wave reductions every kernel ends with (csrc/common.h: wave_sum / wave_max on DPP row operations and
 * v_readlane): 2048 x 256 threads compare them, bit for bit, with the plain butterfly on `rounds` pseudo-random inputs a lane.
 * mismatches[0..3] = lanes that differ for sum<float>, sum<double>, max<float>, max<double> (all 0 on a healthy device).
 * Returns 0 when the test ran. */
int mir_lsq_selftest_reductions(int rounds, int mismatches[4]);
void* mir_lsq_stream_create(void);
void mir_lsq_stream_destroy(void* stream);
int mir_lsq_stream_synchronize(void* stream);
/* "mir_optim_amd <major.minor> (gfx950)". 0.2: the last argument of mir_lsq_batched_kernel_s became the options struct (it was a
 * hipStream_t in 0.1 -- same arity, so an old caller still links: both batched entries answer -1 to an options pointer whose
 * first word is not a plausible struct_size) and mir_optimize_least_squares_batched_s gained it; 0.3: the resident-J options /
 * statistics of part 2 and mir_optim_amd_resident.hpp; 0.4: the batched entries in double (mir_optimize_least_squares_batched_d,
 * mir_lsq_batched_kernel_d, mir_lsq_batched_posvx_d) and double models in launch_batched<Model>. Callers that cache function pointers across versions check this. */
const char* mir_lsq_version(void);

/* =====================================================================================================
 * Part 3 -- a caller of the path: fitSpline (/root/reference/source/mir/optim/fit_splie.d:26-85).
 *
 * Fits the VALUES of a cubic spline at fixed knots x[nx] to scattered points by least squares through the
 * library's own LM entry (n = nx, m = npoints + (lambda == 0)). The spline is mir.interpolate.spline's default
 * configuration (mir-algorithm, un-vendored): C2 cubic, not-a-knot ends, kept in Hermite form (values + first
 * derivatives). Quirks of the reference kept on purpose (its unittest FS:88-141 pins them):
 *   - the smoothness penalty integrates the spline's FIRST derivative at the knots (FS:74, FS:77 index [1]);
 *   - y[m-1] is always overwritten by the penalty term (FS:83): with lambda != 0 the last point is ignored.
 * points: npoints x 2 row-major {abscissa, value}; l, u: bounds on the spline values; dist: optional replacement of
 * the reference's `alias d = "a - b"` (NULL = a - b); splineY (out, nx): fitted values, started from 0 (FS:56-57);
 * splineD (out, nx, optional): first derivatives. Returns MIR_FIT_SPLINE_*; the LM status is in *result (the D
 * function throws for result->status < 0 through `optimize`, LS:175-179, and for TOO_FEW_POINTS, FS:47-51).
 * mir_fit_spline_d / _s run the fit through host callbacks (points in host memory, an optional `dist`);
 * mir_fit_spline_gpu_d / _s, further down, take the points as a DEVICE array and evaluate the residuals in kernels.
 * ===================================================================================================== */
enum { MIR_FIT_SPLINE_OK = 0, MIR_FIT_SPLINE_TOO_FEW_POINTS = 1, MIR_FIT_SPLINE_BAD_ARGUMENT = 2 };

int mir_fit_spline_d(const mir_least_squares_settings_d* settings, size_t npoints, const double* points, size_t nx,
                     const double* x, const double* l, const double* u, double lambda, double (*dist)(double, double),
                     double* splineY, double* splineD, mir_least_squares_result_d* result);
int mir_fit_spline_s(const mir_least_squares_settings_s* settings, size_t npoints, const float* points, size_t nx,
                     const float* x, const float* l, const float* u, float lambda, float (*dist)(float, float),
                     float* splineY, float* splineD, mir_least_squares_result_s* result);
/* the residual function fitSpline minimises (FS:60-84), exposed so that tests can hand the same function to the oracle */
void mir_fit_spline_residuals_d(size_t npoints, const double* points, size_t nx, const double* x, double lambda,
                                const double* splineY, size_t m, double* y);
/* C2 not-a-knot cubic spline: first derivatives at the knots; value / 1st / 2nd derivative at t (out3[3]) */
void mir_spline_c2_derivatives_d(size_t n, const double* x, const double* y, double* d);
void mir_spline_c2_derivatives_s(size_t n, const float* x, const float* y, float* d);
void mir_spline_eval_d(size_t n, const double* x, const double* y, const double* d, double t, double* out3);
void mir_spline_eval_s(size_t n, const float* x, const float* y, const float* d, float t, float* out3);

/* fitSpline on DEVICE-RESIDENT points (csrc/fit_spline_gpu.hip): the same fit through the GPU-native contract of part 2. The
 * residual function is a set of kernels (csrc/fit_spline_kernels.h) behind the library's own f, fb and -- double --
 * fbRowMajorDiff callbacks with MIR_LSQ_DEVICE_CALLBACKS | MIR_LSQ_FD_BASE_POINT, instead of a single-threaded host pass over
 * all points per evaluation: what a caller with 1e5 .. 1e6 scattered samples and 16 .. 256 knots uses. points: DEVICE,
 * npoints x 2 row-major; x, l, u, splineY, splineD: HOST, as above. Same start (splineY = 0), same m, same quirks, same
 * MIR_FIT_SPLINE_* codes and TOO_FEW_POINTS rule as mir_fit_spline_*; npoints == 0 is BAD_ARGUMENT. There is no `dist`
 * (a host function cannot run in a kernel: callers who replace a - b keep mir_fit_spline_*). From `options` (may be NULL) the
 * entry takes stream (NULL: a stream of its own), workspace, stats / stats_size, trace, variant and the MIR_LSQ_TIME_KERNELS
 * flag; options with comm, fb, fbContext, fbRowMajor or fbRowMajorDiff set are BAD_ARGUMENT (the callbacks are the entry's own;
 * row-sharded fits are out of scope: the penalty row belongs to one rank). Every argument check comes before the first HIP
 * call. The residuals are, bit for bit, those of mir_fit_spline_residuals_d (one statement of the arithmetic for host and
 * device, csrc/spline_c2.h). */
int mir_fit_spline_gpu_d(const mir_least_squares_settings_d* settings, size_t npoints, const double* points, size_t nx,
                         const double* x, const double* l, const double* u, double lambda, const mir_lsq_gpu_options* options,
                         double* splineY, double* splineD, mir_least_squares_result_d* result);
int mir_fit_spline_gpu_s(const mir_least_squares_settings_s* settings, size_t npoints, const float* points, size_t nx,
                         const float* x, const float* l, const float* u, float lambda, const mir_lsq_gpu_options* options,
                         float* splineY, float* splineD, mir_least_squares_result_s* result);
/* Values of a spline in Hermite form (x, y, d: HOST, n >= 1 knots) at count abscissae t (DEVICE) -> out (DEVICE): the value
 * mir_spline_eval_* gives, bit for bit; no derivatives. Enqueued on `stream` (NULL = default stream); the call owns its per-row
 * scratch and synchronises the stream before it frees it. Returns 0, -1 (arguments), -2 (no device), -3 (allocation), -5
 * (a copy or launch failed). */
int mir_spline_eval_gpu_d(size_t n, const double* x, const double* y, const double* d, size_t count, const double* t,
                          double* out, void* stream);
int mir_spline_eval_gpu_s(size_t n, const float* x, const float* y, const float* d, size_t count, const float* t,
                          float* out, void* stream);
/* Unit-level access (tests): the per-fit setup of mir_fit_spline_gpu_* and then exactly the callback a solve would call, on the
 * p value vectors X (HOST, p x nx; uploaded). mode 0: fb -> out (HOST) p x m point-major; mode 1: fbRowMajorDiff, p = 2 nx or
 * 2 nx + 1 -> out m x nx row-major differences, then the m residuals of the last vector when p = 2 nx + 1 (the GPU entry:
 * double only). m = npoints + (lambda == 0). _gpu_eval: points DEVICE; _eval_host: points HOST, the same statements of
 * csrc/spline_c2.h on the CPU, no device needed. mir_fit_spline_factor_*: the factor of the knots the callbacks share,
 * F[5 nx] = [di | up | up2 | f | swap], swap[i] = 1 where elimination step i exchanged rows (all 0 for nx < 4: closed forms).
 * Return 0, -1 (arguments), -2 (no device), -3 (allocation), -5 (a copy or launch failed). */
int mir_fit_spline_gpu_eval_d(size_t npoints, const double* points, size_t nx, const double* x, double lambda, size_t p,
                              const double* X, int mode, double* out);
int mir_fit_spline_gpu_eval_s(size_t npoints, const float* points, size_t nx, const float* x, float lambda, size_t p,
                              const float* X, int mode, float* out);
int mir_fit_spline_eval_host_d(size_t npoints, const double* points, size_t nx, const double* x, double lambda, size_t p,
                               const double* X, int mode, double* out);
int mir_fit_spline_eval_host_s(size_t npoints, const float* points, size_t nx, const float* x, float lambda, size_t p,
                               const float* X, int mode, float* out);
int mir_fit_spline_factor_d(size_t nx, const double* x, double* F);
int mir_fit_spline_factor_s(size_t nx, const float* x, float* F);

#ifdef __cplusplus
}
#endif
#endif /* MIR_OPTIM_AMD_H */
