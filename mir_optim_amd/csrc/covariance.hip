// covariance.hip -- Solver<T>::covariance(): the covariance of the fitted parameters, cov = s^2 inv(J^T J), at a given x.
//
// The J a solve ends with is usually a Broyden-aged approximation, sometimes with pending rank-one terms, so the step makes
// ONE full refresh at x with the function a refresh of the solve calls (full_refresh(), solver_jacobian.hip: the analytic g,
// fd_device() or fd_host() with the same callbacks, fd_batch and clipping of x +- jacobianEpsilon to the bounds, LS:1018-1049,
// then J^T J with jacobian_products(false, ...): the plan's kernel, the all-reduce of the packed buffer over the row shards),
// inverts it on the device (spd_inverse.h) and scales by s^2 = ||f(x)||^2 / (M - n_free). Nothing of the LM loop runs.
//
// A parameter with l_j == u_j is FIXED: the refresh has made its column zero (LS:1045), the mask takes its row and column out
// of the system, and they are 0 in the result. A parameter that merely sits on a bound with l_j < u_j is NOT fixed: its
// difference is one-sided or narrower, as in the solve, and it gets a variance like any other.
//
// The n x n scratch, the output and the mask are carved from the workspace's last solve scratch (SolveScratch of ladder entry
// kChainMax - 1: Pm, A, vec, ivec -- rebuilt by every solve before it is read), so the call allocates nothing of its own.
#include "driver.h"
#include "spd_inverse_launch.h"

namespace mirlsq {

// the device side of covariance(): f(x) and its sum of squares, the refresh, the inverse, the scaling, the read-back
template <typename T>
bool Solver<T>::covariance_steps(uint32_t flags, const unsigned char* fixed_h, uint32_t n_free, T* cov, T* residual_h, int* info_h)
{
    // carve() of workspace.hip gives a ladder entry Pm and A of n x n, vec of 12 n elements and ivec of 2 n int32: the factor, the
    // result, the n scale factors, and -- in ivec -- the mask (n bytes at byte 0) and info (one int at int index n, byte 4 n >= n)
    static_assert(sizeof(int32_t) == 4 && sizeof(int) == 4, "mask and info share the 2 n int32 of SolveScratch::ivec");
    const SolveScratch<T>& sc = B.sc[kChainMax - 1];
    unsigned char* fixed_d = reinterpret_cast<unsigned char*>(sc.ivec);          // n bytes of the 2 n int32
    int* info_d = reinterpret_cast<int*>(sc.ivec) + n;
    if (!eval_f(B.x, xh, y) || !sumsq(y, 0)) return false;               // LS:953, 955 -> B.sum[0], all-reduced
    round_kind = 0;
    if (!full_refresh()) return false;                                   // LS:1008-1052, 1065 -> B.JJ
    if (!ok(hipMemcpyAsync(fixed_d, fixed_h, n, hipMemcpyHostToDevice, stream), "H2D fixed mask")
        || !ok(spd_inverse<T>((int)n, B.JJ, fixed_d, sc.Pm, sc.vec, sc.A, info_d, stream), "covariance: inverse")) return false;
    const bool absolute = (flags & MIR_LSQ_COVARIANCE_ABSOLUTE_SIGMA) != 0;
    // M = the rows of all ranks, through the communicator's all-reduce
    if (comm && !absolute && (!ok(cov_rows<T>(B.sum, m, stream), "covariance: rows") || !allreduce(B.sum + 1, 2, 2))) return false;
    return ok(cov_scale<T>((int)n, sc.A, fixed_d, info_d, B.sum, comm != nullptr && !absolute, (double)m, (double)n_free, absolute, stream),
              "covariance: scale")
        && ok(hipMemcpyAsync(cov, sc.A, (size_t)n * n * sizeof(T), hipMemcpyDeviceToHost, stream), "D2H covariance")
        && ok(hipMemcpyAsync(info_h, info_d, sizeof(int), hipMemcpyDeviceToHost, stream), "D2H info")
        && ok(hipMemcpyAsync(residual_h, B.sum, sizeof(T), hipMemcpyDeviceToHost, stream), "D2H residual")
        && ok(hipStreamSynchronize(stream), "sync");
}

template <typename T>
int Solver<T>::covariance(uint32_t flags, T* cov, T* residual_out, int* info_out)
{
    const auto t_start = std::chrono::steady_clock::now();
    launches_mark = launches_now();
    if (const int bad = invalid_input()) return bad;                     // the validation of run(), LS:930-943
    ret.status = mir_ls_numericError; ret.iterations = 0; ret.fCalls = 0; ret.gCalls = 0;
    if (!device_available()) return mir_ls_numericError;
    // the columns the refresh makes zero: l_j == u_j
    std::vector<unsigned char> fixed_h(n);
    uint32_t n_free = 0;
    for (uint32_t j = 0; j < n; ++j) { fixed_h[j] = lh[j] == uh[j] ? 1 : 0; n_free += fixed_h[j] ? 0u : 1u; }
    int info_h = 0;
    T residual_h = 0;
    bool good = setup();
    if (good) {
        good = covariance_steps(flags, fixed_h.data(), n_free, cov, &residual_h, &info_h);
        close_round();
        if (stats) stats->total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    teardown();
    if (!good) return mir_ls_numericError;
    if (info_out) *info_out = info_h;
    if (residual_out) *residual_out = residual_h;
    return 0;
}

template <typename T>
int covariance_entry(const typename Abi<T>::Settings* settings, size_t m, size_t n, const T* x, const T* l, const T* u,
                     const mir_lsq_gpu_options* opt, void* fctx, typename Abi<T>::F f, void* gctx, typename Abi<T>::G g,
                     void* tmctx, mir_least_squares_thread_manager tm, uint32_t flags, T* cov, T* residual_out, int* info)
{
    if (!settings || !l || !u || !cov || !f) return -1;
    if (!x || n == 0) return mir_ls_badGuess;
    if (n > spd_inverse_max_n<T>()) {
        std::fprintf(stderr, "[mir_optim_amd] covariance: n = %zu is beyond the inverse's %zu\n", n, spd_inverse_max_n<T>());
        return mir_ls_numericError;
    }
    std::vector<T> xc(x, x + n);         // the finite-difference tasks perturb copies of it; the caller's x is never written
    Solver<T> s{};
    s.S = settings; s.m = m; s.n = (uint32_t)n; s.xh = xc.data(); s.lh = l; s.uh = u;
    s.fctx = fctx; s.f = f; s.gctx = gctx; s.g = g; s.tmctx = tmctx; s.tm = tm;
    s.apply_options(opt);
    s.trace = nullptr;                   // (a trace records the passes of the LM loop: there are none)
    const int rc = s.covariance(flags, cov, residual_out, info);
    if (s.stats_user) std::memcpy(s.stats_user, &s.stats_local, s.stats_bytes);
    return rc;
}

#define MIRLSQ_INSTANTIATE(T)                                                                                              \
    template bool Solver<T>::covariance_steps(uint32_t, const unsigned char*, uint32_t, T*, T*, int*);                     \
    template int Solver<T>::covariance(uint32_t, T*, T*, int*);                                                            \
    template int covariance_entry<T>(const Abi<T>::Settings*, size_t, size_t, const T*, const T*, const T*,                \
                                     const mir_lsq_gpu_options*, void*, Abi<T>::F, void*, Abi<T>::G, void*,                \
                                     mir_least_squares_thread_manager, uint32_t, T*, T*, int*);
MIRLSQ_INSTANTIATE(double)
MIRLSQ_INSTANTIATE(float)
#undef MIRLSQ_INSTANTIATE

}  // namespace mirlsq

extern "C" {

int mir_lsq_covariance_gpu_d(const mir_least_squares_settings_d* settings, size_t m, size_t n, const double* x, const double* l,
                             const double* u, const mir_lsq_gpu_options* options, void* fContext, mir_least_squares_function_d f,
                             void* gContext, mir_least_squares_jacobian_d g, void* tmContext, mir_least_squares_thread_manager tm,
                             uint32_t flags, double* cov, double* residual_out, int* info)
{
    return mirlsq::covariance_entry<double>(settings, m, n, x, l, u, options, fContext, f, gContext, g, tmContext, tm, flags, cov,
                                            residual_out, info);
}
int mir_lsq_covariance_gpu_s(const mir_least_squares_settings_s* settings, size_t m, size_t n, const float* x, const float* l,
                             const float* u, const mir_lsq_gpu_options* options, void* fContext, mir_least_squares_function_s f,
                             void* gContext, mir_least_squares_jacobian_s g, void* tmContext, mir_least_squares_thread_manager tm,
                             uint32_t flags, float* cov, float* residual_out, int* info)
{
    return mirlsq::covariance_entry<float>(settings, m, n, x, l, u, options, fContext, f, gContext, g, tmContext, tm, flags, cov,
                                           residual_out, info);
}

}  // extern "C"
