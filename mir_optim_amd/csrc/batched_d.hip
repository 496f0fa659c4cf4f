// batched_d.hip -- the batched one-wavefront-per-problem fit in DOUBLE: this unit instantiates the host layer of batched_host.h
// (and with it launch_batched<Model> and the kernels of ModelExpDecayD, ModelExp3AffineD and ModelExpDecayPad8D) for double and holds the
// extern "C" entries of that precision. The float twin is batched.hip.
#include "batched_host.h"

using namespace mirlsq;

extern "C" {

int mir_lsq_batched_kernel_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model, double* x,
                             const double* lower, const double* upper, const double* t, size_t t_stride, const double* data,
                             mir_least_squares_result_d* results, const mir_lsq_batched_options* options)
{
    return batched_kernel_entry<BuiltinModels<double>>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options);
}

int mir_optimize_least_squares_batched_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model,
                                         double* x, const double* lower, const double* upper,
                                         const double* t, size_t t_stride, const double* data,
                                         mir_least_squares_result_d* results, const mir_lsq_batched_options* options)
{
    return batched_host_entry<BuiltinModels<double>>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options);
}

int mir_lsq_batched_posvx_d(size_t count, size_t n, const double* P, const double* rhs, double* x, int* info, void* stream)
{
    return batched_posvx_entry<double>(count, n, P, rhs, x, info, stream);
}

int mir_lsq_batched_kernel_ex_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model, double* x,
                                const double* lower, const double* upper, const double* t, size_t t_stride, const double* data,
                                mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                                const mir_lsq_batched_extras* extras)
{
    return batched_kernel_entry<BuiltinModels<double>>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options, extras);
}

int mir_optimize_least_squares_batched_ex_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model,
                                            double* x, const double* lower, const double* upper,
                                            const double* t, size_t t_stride, const double* data,
                                            mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                                            const mir_lsq_batched_extras* extras)
{
    return batched_host_entry<BuiltinModels<double>>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options, extras);
}

int mir_lsq_batched_covariance_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model, const double* x,
                                 const double* lower, const double* upper, const double* t, size_t t_stride, const double* data,
                                 const mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                                 const mir_lsq_batched_extras* extras)
{
    return batched_covariance_entry<BuiltinModels<double>>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options, extras);
}

}  // extern "C"
