// batched16_ex_d.hip -- weights and covariance for the batched fit of models with 9 to 16 parameters (double): the WEIGHTED
// k_lm_batched16 instances and the k_batched16_covariance instances of the two built-in models (MIR_LSQ_MODEL16_*) and the
// extern "C" entries that take a mir_lsq_batched_extras. An unweighted fit that only asks for its covariance runs the
// unweighted instance of batched16_d.hip (batched16_plain_enqueue): that unit compiles what it always compiled, this one the
// rest, in parallel.
#include "batched16_host.h"

using namespace mirlsq;

namespace {

template <class Model> struct Batched16ExKernels {
    static bool fit(const BatchedArgs<double>& a, bool weighted, size_t lds, hipStream_t stream)
    {
        if (!weighted) return batched16_plain_enqueue(builtin_model16_id<Model>(), a, lds, stream);
        auto kern = k_lm_batched16<Model, true>;
        if (lds > 48 * 1024
            && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return false;
        hipLaunchKernelGGL(kern, dim3((unsigned)a.count), dim3(64), lds, stream, a);
        return true;
    }
    static bool covariance(const BatchedCovArgs<double>& c, size_t lds, hipStream_t stream)
    {
        return mir_optim_amd::detail::Batched16Kernels<Model>::covariance(c, lds, stream);
    }
};

}  // namespace

extern "C" {

// Both _ex entries check in the order of the n <= 8 ones: model id, options and extras (-1), pointers and t_stride (-1), device (-2)
int mir_lsq_batched16_kernel_ex_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model, double* x,
                                  const double* lower, const double* upper, const double* t, size_t t_stride, const double* data,
                                  mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                                  const mir_lsq_batched_extras* extras)
{
    return with_builtin_model16(model, [&](auto mdl) {
        using Model = decltype(mdl);
        if (!batched_options_plausible(options) || !batched_extras_plausible(extras, m)) return -1;
        if (!batched_has_grad<Model>::value && (batched_options(options).variant & MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN)) return -1;
        if (!S || !x || !lower || !upper || !t || !data || !results || (t_stride != 0 && t_stride != m)) return -1;
        if (count != 0 && !device_available()) return -2;
        const mir_lsq_batched_options o = batched_options(options);
        return mir_optim_amd::detail::launch_batched16_with<Model, Batched16ExKernels<Model>>(S, count, m, x, lower, upper, t, t_stride, data,
                                                                                              results, &o, extras);
    });
}

int mir_optimize_least_squares_batched16_ex_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model, double* x,
                                              const double* lower, const double* upper, const double* t, size_t t_stride,
                                              const double* data, mir_least_squares_result_d* results,
                                              const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return with_builtin_model16(model, [&](auto mdl) {
        using Model = decltype(mdl);
        if (!batched_options_plausible(options) || !batched_extras_plausible(extras, m)) return -1;
        if (!batched_has_grad<Model>::value && (batched_options(options).variant & MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN)) return -1;
        if (!S || !x || !lower || !upper || !t || !data || !results || (t_stride != 0 && t_stride != m)) return -1;
        return batched16_host_model_entry<Model, Batched16ExKernels<Model>>(S, count, m, x, lower, upper, t, t_stride, data, results, options,
                                                                            extras);
    });
}

int mir_lsq_batched16_covariance_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model, const double* x,
                                   const double* lower, const double* upper, const double* t, size_t t_stride, const double* data,
                                   const mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                                   const mir_lsq_batched_extras* extras)
{
    return with_builtin_model16(model, [&](auto mdl) {
        using Model = decltype(mdl);
        mir_lsq_batched_extras e;
        if (!batched_options_plausible(options) || !extras || !mir_optim_amd::detail::batched_extras(extras, m, e) || !e.covariance)
            return -1;
        if (!batched_has_grad<Model>::value && (batched_options(options).variant & MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN)) return -1;
        if (!S || !x || !lower || !upper || !t || !data || !results || (t_stride != 0 && t_stride != m)) return -1;
        if (count != 0 && !device_available()) return -2;
        const mir_lsq_batched_options o = batched_options(options);
        return mir_optim_amd::launch_batched16_covariance<Model, Batched16ExKernels<Model>>(S, count, m, x, lower, upper, t, t_stride, data,
                                                                                            results, &o, extras);
    });
}

}  // extern "C"
