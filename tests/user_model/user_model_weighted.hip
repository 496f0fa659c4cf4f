// A caller's OWN residual model fitted with PER-ROW WEIGHTS, and the COVARIANCE of its fitted parameters, through the public
// device header alone (include/mir_optim_amd_batched.hpp): launch_batched<Model> with a mir_lsq_batched_extras, and
// launch_batched_covariance<Model> on the records of an earlier launch. The model has its own derivative, so both Jacobians
// (MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN and central differences) are exercised; it is written once in the value type and
// instantiated in float and in double.
// Build (mir_optim_amd/build.py, user_model_weighted_lib): hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I<repo>/include
#include "mir_optim_amd_batched.hpp"

// a peak on a sloping baseline, as counted by a detector: p0 exp(-(t - p1)^2 / (2 p2^2)) + p3 + p4 t      (n = 5)
// with counts N_i the caller passes w_i = 1 / sqrt(N_i) (and 0 for the channels that are masked out)
template <class T> struct WeightedPeak {
    using value_type = T;
    static constexpr int n = 5, nb = 0;
    __device__ static void basis(T, T*) {}
    __device__ static T eval(T t, const T*, const T* x)
    {
        const T z = (t - x[1]) / x[2];
        return x[0] * exp(T(-0.5) * z * z) + x[3] + x[4] * t;
    }
    __device__ static void grad(T t, const T*, const T* x, T* g)
    {
        const T z = (t - x[1]) / x[2], e = exp(T(-0.5) * z * z);
        g[0] = e;
        g[1] = x[0] * e * z / x[2];
        g[2] = x[0] * e * z * z / x[2];
        g[3] = T(1);
        g[4] = t;
    }
};

// every pointer, those in `extras` included, is a DEVICE pointer (the contract of mir_lsq_batched_kernel_ex_s / _d)
extern "C" int user_fit_weighted_peak_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, double* x,
                                        const double* lower, const double* upper, const double* t, size_t t_stride,
                                        const double* data, mir_least_squares_result_d* results,
                                        const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return mir_optim_amd::launch_batched<WeightedPeak<double>>(settings, count, m, x, lower, upper, t, t_stride, data, results,
                                                               options, extras);
}
extern "C" int user_fit_weighted_peak_s(const mir_least_squares_settings_s* settings, size_t count, size_t m, float* x,
                                        const float* lower, const float* upper, const float* t, size_t t_stride,
                                        const float* data, mir_least_squares_result_s* results,
                                        const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return mir_optim_amd::launch_batched<WeightedPeak<float>>(settings, count, m, x, lower, upper, t, t_stride, data, results,
                                                              options, extras);
}

// the covariance alone, from the x and the records a fit left on the device
extern "C" int user_weighted_peak_covariance_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, const double* x,
                                               const double* lower, const double* upper, const double* t, size_t t_stride,
                                               const double* data, const mir_least_squares_result_d* results,
                                               const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return mir_optim_amd::launch_batched_covariance<WeightedPeak<double>>(settings, count, m, x, lower, upper, t, t_stride, data,
                                                                          results, options, extras);
}
extern "C" int user_weighted_peak_covariance_s(const mir_least_squares_settings_s* settings, size_t count, size_t m, const float* x,
                                               const float* lower, const float* upper, const float* t, size_t t_stride,
                                               const float* data, const mir_least_squares_result_s* results,
                                               const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return mir_optim_amd::launch_batched_covariance<WeightedPeak<float>>(settings, count, m, x, lower, upper, t, t_stride, data,
                                                                         results, options, extras);
}
