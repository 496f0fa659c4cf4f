// driver.h -- host side of the MI355X-native Levenberg-Marquardt solver: what the translation units of the driver share.
//
// The control flow mirrors optimizeLeastSquaresImplGeneric!T (/root/reference/source/mir/optim/least_squares.d:877-1176,
// cited as LS:nnn) pass for pass -- validation order, Jacobian ageing, Broyden / full refresh, gradient test, damping,
// BOXCQP solve, step guard, trial acceptance, lambda / mu schedule, convergence tests -- but every floating-point
// operation of the loop runs in a HIP kernel. The host only sequences kernels on integer / boolean control state that it
// mirrors from a small device-resident LmState after each decision point.
//
//   abi.hip              the reference's extern(C) symbols (LS:637-799, boxcqp.d:36-50) + the additive entry points
//   workspace.hip        device buffers of one (m, n, element type) problem
//   solver_loop.hip      Solver<T>::run(): the LM loop, rounds, decisions (LS:930-1176)
//   solver_jacobian.hip  Jacobian refresh: finite differences (device / host callbacks, LS:1018-1049), analytic g,
//                        Broyden passes, J^T J / J^T y (LS:999-1065)
//   launch_*.hip         the translation units that instantiate the kernels (jtj_plan.h, broyden_launch.h, solve_launch.h)
//   covariance.hip       Solver<T>::covariance(): one refresh at x, J^T J, its inverse (launch_spd_inverse.hip) -> covariance
//   batched.hip, batched_d.hip   one-wavefront-per-problem batched fits in float / double: the two instances of batched_host.h
//   batched_predict.hip, batched_predict_d.hip   fitted curves and confidence bands of the batched fits (batched_predict.h;
//                        float / double with the 16-wide models): the two instances of batched_predict_host.h
//   comm.hip             row-shard communicators;  unit_entries.hip
//   fit_spline.cpp, fit_spline_gpu.hip   fitSpline, a caller of the path: host callbacks / its residuals as kernels (device points)
//
// There is NO CPU fallback: without a usable HIP device the solve entry points print a diagnostic and return
// status = numericError.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/mir_optim_amd.h"
#include "broyden_launch.h"
#include "comm.h"
#include "common.h"
#include "jtj_plan.h"
#include "solve_launch.h"
#include "solve_types.h"

struct mir_lsq_workspace {
    size_t m = 0, n = 0, elem = 0;
    void* dev = nullptr;       // one device allocation, carved below
    size_t dev_bytes = 0;
    void* ypanel = nullptr;    // lazily allocated FD panel (device mode)
    size_t ypanel_bytes = 0;
    void* ytrial = nullptr;    // kChainMax x m trial residuals (speculative lambda ladder)
    void* ulr = nullptr;       // kLrMax x m pending Broyden columns (broyden_lr.h)
    int device = 0;            // the device the workspace lives on (callbacks' worker threads select it)
    std::vector<hipEvent_t> event_pool;   // MIR_LSQ_TIME_KERNELS: events are created once and reused by later solves
    void* pinned = nullptr;    // small pinned host block (state + trial readback), device-mapped and coherent:
    void* pinned_dev = nullptr;   // ... its device address (the decision kernels write the state mirror directly)
    void* pinned_y = nullptr;  // m-vector staging (host-callback mode), lazily allocated
    void* pinned_J = nullptr;  // m*n staging for host analytic Jacobians, lazily allocated
    // host-callback finite differences (fd_host): the 2n residual vectors of a refresh are written by the caller's f straight
    // into this pinned, point-major panel and copied to the device panel by the copy streams while other columns are
    // still being evaluated; lazily allocated
    void* pinned_panel = nullptr;
    size_t pinned_panel_bytes = 0;
    static constexpr int kCopyStreams = 4;
    hipStream_t copy_stream[kCopyStreams] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t copy_event[kCopyStreams] = {nullptr, nullptr, nullptr, nullptr};
    int num_cu = 256;
    uint32_t solve_epoch = 0;  // solve launches with helper workgroups so far (solve_coop.h: the sync words carry it)
};

namespace mirlsq {

template <typename T> struct Abi;
template <> struct Abi<double> {
    using Settings = mir_least_squares_settings_d;
    using Result = mir_least_squares_result_d;
    using F = mir_least_squares_function_d;
    using G = mir_least_squares_jacobian_d;
    using FB = mir_lsq_batched_function_d;
};
template <> struct Abi<float> {
    using Settings = mir_least_squares_settings_s;
    using Result = mir_least_squares_result_s;
    using F = mir_least_squares_function_s;
    using G = mir_least_squares_jacobian_s;
    using FB = mir_lsq_batched_function_s;
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// settings validation of LS:934-943 (after badGuess / badBounds there): the mir_ls_bad* code of the first check that fails, or 0
template <typename Settings>
int bad_settings(const Settings* S)
{
    using T = decltype(Settings::minStepQuality);
    if (!(0 <= S->minStepQuality && S->minStepQuality < 1)) return mir_ls_badMinStepQuality;
    if (!(0 <= S->goodStepQuality && S->goodStepQuality <= 1)) return mir_ls_badGoodStepQuality;
    if (!(S->minStepQuality < S->goodStepQuality)) return mir_ls_badStepQuality;
    if (!(1 <= S->lambdaIncrease && S->lambdaIncrease <= std::sqrt(Lim<T>::max))) return mir_ls_badLambdaParams;
    if (!(std::sqrt(Lim<T>::min_normal) <= S->lambdaDecrease && S->lambdaDecrease <= 1)) return mir_ls_badLambdaParams;
    return 0;
}

// polite busy-wait step: the architecture's spin hint where there is one
inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    std::atomic_signal_fence(std::memory_order_seq_cst);
#endif
}

bool device_available();       // prints the "no CPU fallback" diagnostic when there is none (workspace.hip)
int query_num_cu();

// ------------------------------------------------------------------------------------------
// device buffers carved from one allocation
// ------------------------------------------------------------------------------------------
template <typename T>
struct Buffers {
    T *J, *y, *mB, *ytmp;
    T *X, *twh;
    T *x, *lower, *upper, *dx, *dx_acc, *trial, *Jy, *JJ, *packed, *partials, *sum;
    LmState<T>* st;
    ChainRec<T>* rec;
    T* slabs;
    T *lrD, *lrvec, *lrpart;   // pending Broyden steps (kLrMax x n), reduced sweep vector, per-workgroup partials
    SolveScratch<T> sc[kChainMax];
    size_t bytes;
};

constexpr int kPartials = 1024;

// workgroups of the entry residual's two-stage sum of squares (Solver::sumsq, LS:955): 4096 rows each, at most kPartials
inline int sumsq_blocks(size_t m)
{
    int nb = (int)((m + 4095) / 4096);
    if (nb > kPartials) nb = kPartials;
    return nb < 1 ? 1 : nb;
}

// the interval widths of k_fd_points with the same arithmetic on the host (LS:1027-1033): twh[j] = min(x_j + eps, u_j) - max(x_j - eps, l_j)
template <typename T>
inline void fd_widths(const T* x, const T* lower, const T* upper, T eps, size_t n, T* twh)
{
    for (size_t j = 0; j < n; ++j) {
        const T save = x[j];
        T xmh = save - eps, xph = save + eps;
        xmh = std::fmax(xmh, lower[j]);
        xph = std::fmin(xph, upper[j]);
        twh[j] = xph - xmh;
    }
}

template <typename T> Buffers<T> carve(void* base, size_t m, size_t n, int num_cu);
template <typename T> mir_lsq_workspace* workspace_create(size_t m, size_t n);
void workspace_destroy(mir_lsq_workspace* ws);

// ------------------------------------------------------------------------------------------
// the solver
// ------------------------------------------------------------------------------------------
struct EventPair { hipEvent_t a, b; int kind; };   // kind: 0 jtj, 1 Broyden pass, 2 solve, 3 FD jtj, 4 FD callbacks, 5 trial callbacks

template <typename T>
struct Solver {
    using Settings = typename Abi<T>::Settings;
    using Result = typename Abi<T>::Result;
    using F = typename Abi<T>::F;
    using G = typename Abi<T>::G;
    using FB = typename Abi<T>::FB;

    const Settings* S;
    size_t m;
    uint32_t n;
    T* xh;                 // caller's x (host), updated in place on accepted steps (LS:1135)
    const T *lh, *uh;
    void* fctx; F f;
    void* gctx; G g;
    void* tmctx; mir_least_squares_thread_manager tm;
    void* fbctx; FB fb;
    FB fbr = nullptr;          // batched residual callback writing Y row-major (m x p): the pair panel of the fused FD kernels
    FB fbd = nullptr;          // batched residual callback writing the m x n row-major DIFFERENCE panel (fbRowMajorDiff)
    int fd_fused = 0;          // 1: the (+h, -h) pair panel, 2: the difference panel of this refresh is in ws->ypanel and J has not been filled yet
    // J0 lives UNSCALED in ws->ypanel, scaled by B.twh: the last refresh was the fused kernel of the difference panel and did not
    // write B.J (a.Jout = nullptr) -- the Broyden sweeps and the flush read the panel and scale what they load (lr_sweep, lr_flush_scaled).
    // Set by jacobian_products() for the fd_fused == 2 refresh of a solve with read-only Broyden passes (lowrank, n <=
    // kLrScaledMaxN, no MIR_LSQ_VARIANT_FD_WRITE_J); cleared by the flush, which materialises B.J, and by every other refresh.
    bool j0_in_panel = false;
    const T* lr_j0() const { return j0_in_panel ? static_cast<const T*>(ws->ypanel) : B.J; }
    const T* lr_twh() const { return j0_in_panel ? B.twh : nullptr; }
    // MIR_LSQ_FD_BASE_POINT (fd_entry, solver_jacobian.hip): the caller's fbd also takes p = 2n + 1, so the entry residual f(x0)
    // and the first refresh's difference panel -- same x0 -- come from ONE call. fd_entry_ready: that panel is in ws->ypanel and
    // the first pass's fd_device() has only its bookkeeping left; a solve that ends before that pass discards it.
    bool fd_base_point = false;
    bool fd_entry_ready = false;
    size_t fd_entry_event = (size_t)-1;   // the timed bracket of that call (MIR_LSQ_TIME_KERNELS), dropped with a discarded panel
    uint64_t launches_early = 0;      // launched at entry on behalf of the first refresh round (k_fd_points): booked to that round,
    uint64_t launches_held = 0;       // not to the entry -- held here from the entry's close_round() to the round's
    int sums_pending = 0;      // > 0: the trial sums of this round are still k_lr_sumsq's stage-1 partials (k_decide_chain finishes them)
    uint32_t fd_batch;
    bool device_cb;
    bool time_kernels;
    mir_lsq_comm* comm;
    mir_lsq_stats* stats;
    mir_lsq_trace* trace = nullptr;

    hipStream_t stream = nullptr;
    bool own_stream = false;
    mir_lsq_workspace* ws = nullptr;
    bool own_ws = false;
    Buffers<T> B;
    JtjPlan plan;
    LmSettingsDev<T> sd;
    // A/B switches (mir_lsq_gpu_options.variant, MIR_LSQ_VARIANT_*): 0 = product path. Broyden passes keep J and carry the
    // updates as pending rank-one terms (broyden_lr.h); BROYDEN_REWRITE selects the kernels that rewrite J every pass;
    // bits 16..20 the number of pending terms after which they are folded into J
    uint32_t variant = 0;
    bool dbg_solve = false, no_speculation = false, lowrank = true, no_null_skip = false, host_profile = false;
    mir_lsq_stats stats_local{};      // the solve works on this image; stats_bytes of it go back to the caller's struct
    mir_lsq_stats* stats_user = nullptr;
    size_t stats_bytes = 0;
    uint64_t launches_mark = 0;       // tl_launches at the start of the round being accounted (mir_lsq_stats.round_launches)
    int round_kind = -1;
    uint64_t launches_excluded = 0;   // of the launches since the mark: those that belong to no round (flush + resynchronisation)
    std::atomic<uint64_t> worker_launches{0};   // kernels launched on behalf of this solve by OTHER threads (the thread manager's
                                                // workers, FD_HOST_COLUMNS): tl_launches is per thread and does not see them
    int lr_cap = kLrMax;
    int lr_k = 0;
    int device = 0, caller_device = -1;
    // the reference swaps the contents of y and mBuffer on acceptance (LS:1136); here the two device buffers swap roles.
    // Everything that touches them goes through these members (never through B.y / B.mB directly).
    T* y = nullptr;
    T* mB = nullptr;
    T* fr = nullptr;     // third m-vector: the trial residual of a round goes here; accepting rotates (y, mB, fr) <- (fr, y, mB)
    // null steps (trial == x bit for bit; kFlagNullStep): once a round ended on one, the next round's solves are looked
    // at before the callbacks are launched, and when every entry is a null step nothing is evaluated
    bool has_bounds = true;    // some lower / upper entry is finite (set in enter()); MIR_LSQ_VARIANT_SOLVE_BOUNDED forces the full kernel
    bool tail_null = false;
    // ---- the fused round (solver_loop.hip, setup() and enqueue_fused_tail()): behind a round's one trial residual the next
    // pass's Broyden sweep runs speculatively and carries the trial's sum of squares; one kernel then decides the trial and, if
    // it is accepted without any exit test firing, applies the pass's n x n side and solves the next system. Results are
    // bit-identical with the one-by-one rounds (MIR_LSQ_VARIANT_NO_PIPELINE; tests/test_gpu_lm.py).
    bool fused = false;            // allowed at all for this solve (see setup())
    bool spec_enqueue = false;     // set while the kernels of the pass run ahead are being enqueued (their events are tagged)
    size_t spec_events_from = 0;   // events of the pass run ahead start here
    bool big_solve = false;    // n > 256 (or MIR_LSQ_VARIANT_SOLVE_GENERIC): the any-n solve kernel
    bool coop_disabled = false;   // helper workgroups timed out once in this solve: one workgroup per entry from now on

    LmState<T>* st_h;      // pinned mirror of the decision point being processed (one of st_slot[])
    LmState<T>* st_slot[2] = {nullptr, nullptr};     // the two mirrors, host and device addresses
    LmState<T>* st_slot_d[2] = {nullptr, nullptr};
    T* x_slot[2] = {nullptr, nullptr};               // accepted point of decision point seq at x_slot[seq & 1]
    T* x_slot_d[2] = {nullptr, nullptr};
    T* x_h = nullptr;              // x mirror of the decision point being processed
    uint32_t seq = 0;              // decision points enqueued so far
    T* trial_h;            // pinned, n
    std::vector<T> twh_h;
    std::vector<EventPair> events;
    Result ret;

    // ---- the LM loop (solver_loop.hip): what run() carries from pass to pass, and what one pass works out for itself
    struct Loop {
        bool fConverged = false, needJacobian = true, last_rejected = false;   // LS:956, 959
        bool spec_live = false;            // the Jacobian side and the solve of the round at the top of the loop have run already (fused round)
        bool spec_predict = true;          // the last first trial after a Jacobian update was accepted
        bool speculate = false;            // ladder trials: one fb call, or ks calls of f
        T mu = 1;
        uint32_t age = 0, maxAge = 0;      // LS:945
    } lp;
    struct Round {
        T* ytr;                            // the trial residuals: the free buffer, or the ladder's ks vectors
        int ks = 1;                        // ladder entries of the round, lam[0 .. ks)
        T lam[kChainMax];
        bool newJacobian = false, lambda_from_state = false, skip_eval = false;
        bool solve_enqueued = false;       // the previous round's fused kernel has solved already
        bool fuse = false;                 // this round's decision is the head of a fused kernel
    };
    // what a stage answers: on with this pass, on to the next pass, stop with ret.status, or a device error
    enum class Flow { go, next, stop, error };
    Flow stop(int status) { ret.status = status; return Flow::stop; }

    // host-callback finite differences (reference thread-manager contract, LS:1019-1048)
    struct Slot { T* p = nullptr; T* yp = nullptr; T* ym = nullptr; };
    std::vector<Slot> slots;
    std::vector<int> slot_count;
    std::mutex fd_mutex;
    std::atomic<bool> fd_failed{false};
    bool fd_panel_mode = false;        // this refresh stages through the pinned point-major panel (fd_host)
    std::atomic<uint32_t> fd_streams_used{0};   // bit k: copy stream k carries copies of this refresh
    std::atomic<uint64_t> fd_f_ns{0};  // wall time inside the caller's f, summed over the tasks (statistics)
    std::atomic<uint32_t> fd_tasks_run{0};   // tasks the manager has run in this refresh: every i in [0, n) exactly once (LS:575-578)

    // MIR_LSQ_VARIANT_HOST_PROFILE: host wall time per category of runtime call, printed at teardown (diagnostic)
    double hp_ms[6] = {0, 0, 0, 0, 0, 0};   // 0 events, 1 all-reduce calls, 2 callbacks, 3 sync/readback, 4 launches (solve), 5 max single
    struct HpScope {
        Solver* s; int cat; std::chrono::steady_clock::time_point t0;
        HpScope(Solver* s_, int c) : s(s_), cat(c) { if (s->host_profile) t0 = std::chrono::steady_clock::now(); }
        ~HpScope() {
            if (!s->host_profile) return;
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            s->hp_ms[cat] += ms;
            if (ms > s->hp_ms[5]) s->hp_ms[5] = ms;
        }
    };

    bool ok(hipError_t e, const char* what)
    {
        if (e == hipSuccess) return true;
        std::fprintf(stderr, "[mir_optim_amd] %s failed: %s\n", what, hipGetErrorName(e));
        return false;
    }
    // kernels launched for this solve so far: this thread's counter + what the thread manager's workers launched
    uint64_t launches_now() const { return tl_launches + worker_launches.load(std::memory_order_relaxed); }
    void close_round()
    {
        const uint64_t now = launches_now();
        uint64_t cnt = now - launches_mark;
        if (round_kind < 0) { cnt -= launches_early; launches_held += launches_early; launches_early = 0; }
        else { cnt += launches_held; launches_held = 0; }
        if (stats) {
            stats->library_launches += cnt;
            if (round_kind >= 0) { stats->round_launches[round_kind] += cnt - launches_excluded; stats->rounds[round_kind]++; }
        }
        launches_mark = now;
        launches_excluded = 0;
        round_kind = -1;
    }
    void ev_begin(int kind);
    void ev_end();
    // validation, LS:930-943 (quirk Q9), of the solve and of the covariance step -- needs no device: the status, or 0
    int invalid_input() const
    {
        if (m == 0 || n == 0) return mir_ls_badGuess;
        for (uint32_t i = 0; i < n; ++i) if (!(-Lim<T>::inf() < xh[i] && xh[i] < Lim<T>::inf())) return mir_ls_badGuess;
        for (uint32_t i = 0; i < n; ++i) if (!(lh[i] <= xh[i]) || !(xh[i] <= uh[i])) return mir_ls_badBounds;
        return bad_settings(S);
    }

    // ---- solver_loop.hip
    bool setup();
    void teardown();
    bool eval_f(const T* x_dev, const T* x_host, T* y_dev);
    bool sumsq(const T* v, int slot);
    bool trial_sums(const T* v, int count, size_t vstride);
    bool allreduce(T* buf, size_t count, int kind);
    void trace_emit(int event, uint32_t iterations, T lambda, T residual, T trial_residual, T dx_dot);
    bool trace_round(int ks, T residual_before, uint32_t iterations_before);
    bool wait_state(uint32_t expect);
    void print_solve_dbg(bool fused_round);
    LmSolveArgs<T> solve_args(int ks, const T* lam, bool check_grad, bool lambda_from_state);
    DecideArgs<T> decide_args(int ks, bool check_grad, bool lambda_from_state);
    bool enqueue_decide(int ks, bool check_grad, bool lambda_from_state, const T* sum_v = nullptr);
    bool enqueue_fused_tail(const T* ytr, bool check_grad, bool lambda_from_state);
    void commit_spec_round();
    void drop_spec_round();
    bool enter();
    Flow top_of_pass();
    bool adopt_spec_round(Round& r), jacobian_side(Round& r);
    void ladder(Round& r);
    bool solve_round(Round& r), trial_residuals(Round& r), decide(Round& r);
    Flow book(Round& r);
    Flow pass();
    Result run();
    void apply_options(const mir_lsq_gpu_options* opt);

    // ---- solver_jacobian.hip
    bool broyden_lowrank(const T* y_dev, const T* yold_dev);
    bool plain_products(const T* y_vec);
    bool unpack_in_reduce(JtjOp op) const { return !comm && jtj_unpacks(plan, op); }
    JtjUnpack<T> unpack_target() { JtjUnpack<T> u; u.JJ = B.JJ; u.Jy = B.Jy; return u; }
    bool run_products(JtjOp op, const JtjArgs<T>& a, int kind, const char* what);
    bool jacobian_products(bool broyden, const T* y_dev, const T* yold_dev);
    bool full_refresh();
    bool fd_panel(size_t& pb, bool& use_diff);
    void fd_widths_host();
    bool fd_entry(bool& done);
    void fd_entry_discard();
    bool fd_device();
    static void fd_task_trampoline(mir_least_squares_task task, uint32_t totalThreads, uint32_t threadId, uint32_t j);
    void fd_task(uint32_t totalThreads, uint32_t threadId, uint32_t j);
    bool fd_host_prepare_panel();
    bool fd_host();
    bool analytic_jacobian();

    // ---- covariance.hip: cov = s^2 inv(J^T J) of ONE full refresh at x, nothing of the LM loop
    bool covariance_steps(uint32_t flags, const unsigned char* fixed_h, uint32_t n_free, T* cov, T* residual_h, int* info_h);
    int covariance(uint32_t flags, T* cov, T* residual_out, int* info_out);
};

// the one entry every solve goes through (solver_loop.hip; instantiated for double and float)
template <typename T>
typename Abi<T>::Result solve_entry(const typename Abi<T>::Settings* settings, size_t m, size_t n, T* x, const T* l,
                                    const T* u, const mir_lsq_gpu_options* opt, void* fctx, typename Abi<T>::F f,
                                    void* gctx, typename Abi<T>::G g, void* tmctx, mir_least_squares_thread_manager tm);
// mir_lsq_covariance_gpu_* (covariance.hip)
template <typename T>
int covariance_entry(const typename Abi<T>::Settings* settings, size_t m, size_t n, const T* x, const T* l, const T* u,
                     const mir_lsq_gpu_options* opt, void* fctx, typename Abi<T>::F f, void* gctx, typename Abi<T>::G g,
                     void* tmctx, mir_least_squares_thread_manager tm, uint32_t flags, T* cov, T* residual_out, int* info);

}  // namespace mirlsq
