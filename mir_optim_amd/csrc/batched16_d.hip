// batched16_d.hip -- the batched one-wavefront-per-problem fit for models with 9 to 16 parameters (double; batched16_kernel.h,
// launch_batched16<Model> of include/mir_optim_amd_batched.hpp): the k_lm_batched16 instances of the two built-in models
// (MIR_LSQ_MODEL16_*), their extern "C" entries and the unit entry of the J^T J stage. A unit of its own, so that batched_d.hip
// compiles the device code it always compiled and the build stays parallel. The weighted instances, the covariance kernel and
// the entries that take weights and covariance are in batched16_ex_d.hip; the host layer of both is batched16_host.h.
#include "batched16_host.h"

using namespace mirlsq;

namespace {

// NULL, or a plausible struct that asks for neither weights nor covariance (those have entries of their own, the _ex entries of
// batched16_ex_d.hip: these two answer -1, as they did before those existed). Its flags pass: MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM
// needs no other kernel instance.
bool extras16_acceptable(const mir_lsq_batched_extras* extras, size_t m)
{
    mir_lsq_batched_extras e;
    return mir_optim_amd::detail::batched_extras(extras, m, e) && !e.weights && !e.covariance;
}
// what such an extras hands on to the launch: its per-problem-bounds bit and nothing else; false: nothing to hand on
bool extras16_flags_only(const mir_lsq_batched_extras* extras, size_t m, mir_lsq_batched_extras& f)
{
    mir_lsq_batched_extras e;
    (void)mir_optim_amd::detail::batched_extras(extras, m, e);
    f = mir_lsq_batched_extras{};
    f.struct_size = sizeof f;
    f.flags = e.flags & MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM;
    return f.flags != 0;
}

// the kernels of this unit: the unweighted fit and nothing else
template <class Model> struct Batched16PlainKernels {
    static bool fit(const BatchedArgs<double>& a, bool weighted, size_t lds, hipStream_t stream)
    {
        if (weighted) return false;
        auto kern = k_lm_batched16<Model>;
        if (lds > 48 * 1024
            && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return false;
        hipLaunchKernelGGL(kern, dim3((unsigned)a.count), dim3(64), lds, stream, a);
        return true;
    }
    static bool covariance(const BatchedCovArgs<double>&, size_t, hipStream_t) { return false; }
};

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
        mir_lsq_batched_extras f;
        const bool per_problem = extras16_flags_only(extras, m, f);
        return mir_optim_amd::detail::launch_batched16_with<decltype(mdl), Batched16PlainKernels<decltype(mdl)>>(
            S, count, m, x, lower, upper, t, t_stride, data, results, &o, per_problem ? &f : nullptr);
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
        mir_lsq_batched_extras f;
        const bool per_problem = extras16_flags_only(extras, m, f);
        return batched16_host_model_entry<decltype(mdl), Batched16PlainKernels<decltype(mdl)>>(S, count, m, x, lower, upper, t, t_stride,
                                                                                               data, results, options,
                                                                                               per_problem ? &f : nullptr);
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

// (after the entries: the kernels are then instantiated in the order in which this unit always emitted them)
bool mirlsq::batched16_plain_enqueue(int model, const BatchedArgs<double>& a, size_t lds, hipStream_t stream)
{
    return with_builtin_model16(model, [&](auto mdl) { return (int)Batched16PlainKernels<decltype(mdl)>::fit(a, false, lds, stream); }) == 1;
}
