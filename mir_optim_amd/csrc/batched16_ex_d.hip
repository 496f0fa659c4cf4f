// batched16_ex_d.hip -- weights and covariance for the batched fit of models with 9 to 16 parameters (double): the WEIGHTED
// k_lm_batched16 instances and the k_batched16_covariance instances of the two built-in models (MIR_LSQ_MODEL16_*) and the
// extern "C" entries that take a mir_lsq_batched_extras. An unweighted fit that only asks for its covariance runs the
// unweighted instance of batched16_d.hip (batched16_plain_enqueue): that unit compiles what it always compiled, this one the
// rest, in parallel.
#include "batched_host.h"

using namespace mirlsq;

namespace {

template <class Model> struct Batched16ExKernels {
    static bool fit(const BatchedArgs<double>& a, bool weighted, size_t lds, hipStream_t stream)
    {
        if (!weighted) return batched16_plain_enqueue(builtin_model16_id<Model>(), a, lds, stream);
        return mir_optim_amd::detail::launch_kernel(k_lm_batched16<Model, true>, dim3((unsigned)a.count), dim3(64), lds, stream, a);
    }
    static bool covariance(const BatchedCovArgs<double>& c, size_t lds, hipStream_t stream)
    {
        return mir_optim_amd::detail::Batched16Kernels<Model>::covariance(c, lds, stream);
    }
};
using Models = BuiltinModels16<Batched16ExKernels, false>;

}  // namespace

extern "C" {

int mir_lsq_batched16_kernel_ex_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model, double* x,
                                  const double* lower, const double* upper, const double* t, size_t t_stride, const double* data,
                                  mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                                  const mir_lsq_batched_extras* extras)
{
    return batched_kernel_entry<Models>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options, extras);
}

int mir_optimize_least_squares_batched16_ex_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model, double* x,
                                              const double* lower, const double* upper, const double* t, size_t t_stride,
                                              const double* data, mir_least_squares_result_d* results,
                                              const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return batched_host_entry<Models>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options, extras);
}

int mir_lsq_batched16_covariance_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model, const double* x,
                                   const double* lower, const double* upper, const double* t, size_t t_stride, const double* data,
                                   const mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                                   const mir_lsq_batched_extras* extras)
{
    return batched_covariance_entry<Models>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options, extras);
}

}  // extern "C"
