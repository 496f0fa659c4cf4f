// batched16_d.hip -- the batched one-wavefront-per-problem fit for models with 9 to 16 parameters (double; batched16_kernel.h,
// launch_batched16<Model> of include/mir_optim_amd_batched.hpp): the k_lm_batched16 instances of the two built-in models
// (MIR_LSQ_MODEL16_*), their extern "C" entries and the unit entry of the J^T J stage. A unit of its own, so that batched_d.hip
// compiles the device code it always compiled and the build stays parallel.
#include "batched_host.h"

using namespace mirlsq;

namespace {

// THE dispatch from a MIR_LSQ_MODEL16_* id to the built-in model type: f(Model{}), or -1 for any other id (0, 1 and 2 included:
// those are models of the n <= 8 entries)
template <class F>
int with_builtin_model16(int id, F&& f)
{
    switch (id) {
    case kModel16ExpHarm16: return f(BuiltinModel16<kModel16ExpHarm16>::type{});
    case kModel16Gauss3Affine: return f(BuiltinModel16<kModel16Gauss3Affine>::type{});
    }
    return -1;
}

// NULL, or a plausible struct that asks for neither weights nor covariance (both are follow-ups of this entry: -1 until then)
bool extras16_acceptable(const mir_lsq_batched_extras* extras, size_t m)
{
    mir_lsq_batched_extras e;
    return mir_optim_amd::detail::batched_extras(extras, m, e) && !e.weights && !e.covariance;
}

template <class Model>
int batched16_host_model_entry(const mir_least_squares_settings_d* S, size_t count, size_t m, double* x, const double* lower,
                               const double* upper, const double* t, size_t t_stride, const double* data,
                               mir_least_squares_result_d* results, const mir_lsq_batched_options* options)
{
    using Result = mir_least_squares_result_d;
    constexpr size_t n = Model::n;
    for (size_t i = 0; i < count; ++i) {       // defaults of LeastSquaresResult!T, LS:132-142
        results[i].status = mir_ls_numericError; results[i].iterations = results[i].fCalls = results[i].gCalls = 0;
        results[i].residual = Lim<double>::inf(); results[i].lambda = 0;
    }
    if (count == 0) return 0;
    const int bad = bad_settings(S);           // common to all problems (the code is reported per problem)
    if (!device_available()) return -2;
    if (m == 0 || mir_optim_amd::batched16_lds_bytes<Model>(m) > mir_optim_amd::kBatchedLdsLimit) {
        std::fprintf(stderr, "[mir_optim_amd] batched16 entry: m = %zu does not fit one wave's LDS slice (m <= %zu)\n", m,
                     mir_optim_amd::kBatched16MaxRows);
        return -3;
    }
    if (bad) {
        for (size_t i = 0; i < count; ++i) results[i].status = bad;
        return 0;
    }
    mir_lsq_batched_options o = batched_options(options);
    o.stream = nullptr;
    // one allocation: the arrays, the records and the model's per-row basis table
    const size_t basis_b = mir_optim_amd::batched_basis_floats<Model>(count, m, t_stride) * sizeof(double);
    const size_t tb = (t_stride ? count : 1) * m * sizeof(double), db = count * m * sizeof(double), xb = count * n * sizeof(double);
    char* base = nullptr;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o_ = off; off = align_up(off + bytes, 256); return o_; };
    const size_t ot = take(tb), od = take(db), ox = take(xb), ol = take(n * sizeof(double)), ou = take(n * sizeof(double)),
                 orr = take(count * sizeof(Result)), obasis = take(basis_b);
    if (hipMalloc((void**)&base, off) != hipSuccess) return -4;
    o.basis = basis_b ? (float*)(base + obasis) : nullptr;      // the C member is float*; it holds doubles here
    o.basis_bytes = basis_b;
    bool good = hipMemcpy(base + ot, t, tb, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + od, data, db, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ox, x, xb, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ol, lower, n * sizeof(double), hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ou, upper, n * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    good = good
        && mir_optim_amd::launch_batched16<Model>(S, count, m, (double*)(base + ox), (const double*)(base + ol), (const double*)(base + ou),
                                                  (const double*)(base + ot), t_stride, (const double*)(base + od),
                                                  (Result*)(base + orr), &o) == 0
        && hipDeviceSynchronize() == hipSuccess
        && hipMemcpy(results, base + orr, count * sizeof(Result), hipMemcpyDeviceToHost) == hipSuccess
        && hipMemcpy(x, base + ox, xb, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(base);
    return good ? 0 : -5;
}

}  // namespace

extern "C" {

int mir_lsq_batched16_kernel_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model, double* x,
                               const double* lower, const double* upper, const double* t, size_t t_stride, const double* data,
                               mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                               const mir_lsq_batched_extras* extras)
{
    return with_builtin_model16(model, [&](auto mdl) {
        if (!batched_options_plausible(options) || !extras16_acceptable(extras, m)) return -1;
        if (!batched_has_grad<decltype(mdl)>::value && (batched_options(options).variant & MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN)) return -1;
        if (!S || !x || !lower || !upper || !t || !data || !results || (t_stride != 0 && t_stride != m)) return -1;
        if (count != 0 && !device_available()) return -2;
        const mir_lsq_batched_options o = batched_options(options);
        return mir_optim_amd::launch_batched16<decltype(mdl)>(S, count, m, x, lower, upper, t, t_stride, data, results, &o);
    });
}

int mir_optimize_least_squares_batched16_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model, double* x,
                                           const double* lower, const double* upper, const double* t, size_t t_stride,
                                           const double* data, mir_least_squares_result_d* results,
                                           const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return with_builtin_model16(model, [&](auto mdl) {
        if (!batched_options_plausible(options) || !extras16_acceptable(extras, m)) return -1;
        if (!batched_has_grad<decltype(mdl)>::value && (batched_options(options).variant & MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN)) return -1;
        if (!S || !x || !lower || !upper || !t || !data || !results || (t_stride != 0 && t_stride != m)) return -1;
        return batched16_host_model_entry<decltype(mdl)>(S, count, m, x, lower, upper, t, t_stride, data, results, options);
    });
}

int mir_lsq_batched16_jtj_d(size_t count, size_t m, size_t n, const double* J, const double* y, double* JJ, double* Jy, void* stream)
{
    if (!J || !y || !JJ || !Jy || n < 1 || n > (size_t)kW16) return -1;
    if (count == 0) return 0;
    const size_t lds = ((size_t)(kW16 + 1) * m + kBatched16TileDoubles) * sizeof(double);
    if (m == 0 || lds > mir_optim_amd::kBatchedLdsLimit) return -3;
    if (!device_available()) return -2;
    if (lds > 48 * 1024
        && hipFuncSetAttribute(reinterpret_cast<const void*>(k_batched16_jtj<>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -5;
    hipLaunchKernelGGL(k_batched16_jtj<>, dim3((unsigned)count), dim3(64), lds, static_cast<hipStream_t>(stream), (int)count, (int)m, (int)n,
                       J, y, JJ, Jy);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // extern "C"
