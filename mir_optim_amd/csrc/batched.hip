// batched.hip -- the batched one-wavefront-per-problem fit in FLOAT: this unit instantiates the host layer of batched_host.h
// (and with it launch_batched<Model> and the kernels of ModelExpDecay, ModelExp3Affine and ModelExpDecayPad8) for float and holds the
// extern "C" entries of that precision. The double twin is batched_d.hip.
#include "batched_host.h"

using namespace mirlsq;

extern "C" {

int mir_lsq_batched_kernel_s(const mir_least_squares_settings_s* S, size_t count, size_t m, int model, float* x,
                             const float* lower, const float* upper, const float* t, size_t t_stride, const float* data,
                             mir_least_squares_result_s* results, const mir_lsq_batched_options* options)
{
    return batched_kernel_entry<BuiltinModels<float>>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options);
}

int mir_optimize_least_squares_batched_s(const mir_least_squares_settings_s* S, size_t count, size_t m, int model,
                                         float* x, const float* lower, const float* upper,
                                         const float* t, size_t t_stride, const float* data,
                                         mir_least_squares_result_s* results, const mir_lsq_batched_options* options)
{
    return batched_host_entry<BuiltinModels<float>>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options);
}

int mir_lsq_batched_posvx_s(size_t count, size_t n, const float* P, const float* rhs, float* x, int* info, void* stream)
{
    return batched_posvx_entry<float>(count, n, P, rhs, x, info, stream);
}

int mir_lsq_batched_kernel_ex_s(const mir_least_squares_settings_s* S, size_t count, size_t m, int model, float* x,
                                const float* lower, const float* upper, const float* t, size_t t_stride, const float* data,
                                mir_least_squares_result_s* results, const mir_lsq_batched_options* options,
                                const mir_lsq_batched_extras* extras)
{
    return batched_kernel_entry<BuiltinModels<float>>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options, extras);
}

int mir_optimize_least_squares_batched_ex_s(const mir_least_squares_settings_s* S, size_t count, size_t m, int model,
                                            float* x, const float* lower, const float* upper,
                                            const float* t, size_t t_stride, const float* data,
                                            mir_least_squares_result_s* results, const mir_lsq_batched_options* options,
                                            const mir_lsq_batched_extras* extras)
{
    return batched_host_entry<BuiltinModels<float>>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options, extras);
}

int mir_lsq_batched_covariance_s(const mir_least_squares_settings_s* S, size_t count, size_t m, int model, const float* x,
                                 const float* lower, const float* upper, const float* t, size_t t_stride, const float* data,
                                 const mir_least_squares_result_s* results, const mir_lsq_batched_options* options,
                                 const mir_lsq_batched_extras* extras)
{
    return batched_covariance_entry<BuiltinModels<float>>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options, extras);
}

}  // extern "C"
