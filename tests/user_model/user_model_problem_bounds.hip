// A caller's OWN residual model fitted with a box PER PROBLEM, through the public device header alone
// (include/mir_optim_amd_batched.hpp): launch_batched_bounded<Model> with MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM in the flags of
// the trailing mir_lsq_batched_extras. `lower` and `upper` then hold count x n values, row k being the box of problem k: here a
// window for the peak position around each spectrum's own maximum, and -- for a caller who knows a spectrum's baseline -- that
// parameter held fixed (lower == upper in that problem's row). With extras->covariance the covariance of the fitted parameters
// follows on the same stream; the row and column of a fixed parameter are 0 there.
// Build (mir_optim_amd/build.py, user_model_problem_bounds_lib): hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I<repo>/include
#include "mir_optim_amd_batched.hpp"

// one Gaussian peak on a constant baseline: p0 exp(-((t - p1) / p2)^2 / 2) + p3      (n = 4)
template <class T> struct PeakOnBaseline {
    using value_type = T;
    static constexpr int n = 4, nb = 0;
    __device__ static void basis(T, T*) {}
    __device__ static T eval(T t, const T*, const T* x)
    {
        const T z = (t - x[1]) / x[2];
        return x[0] * exp(T(-0.5) * z * z) + x[3];
    }
    __device__ static void grad(T t, const T*, const T* x, T* g)
    {
        const T z = (t - x[1]) / x[2], e = exp(T(-0.5) * z * z);
        g[0] = e;
        g[1] = x[0] * e * z / x[2];
        g[2] = x[0] * e * z * z / x[2];
        g[3] = T(1);
    }
};

// every pointer, those in `extras` included, is a DEVICE pointer (the contract of mir_lsq_batched_kernel_ex_s / _d); the caller
// sets MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM in extras->flags and passes count x 4 values in lower and in upper
extern "C" int user_fit_peak_window_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, double* x,
                                      const double* lower, const double* upper, const double* t, size_t t_stride,
                                      const double* data, mir_least_squares_result_d* results,
                                      const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return mir_optim_amd::launch_batched_bounded<PeakOnBaseline<double>>(settings, count, m, x, lower, upper, t, t_stride, data,
                                                                         results, options, extras);
}
extern "C" int user_fit_peak_window_s(const mir_least_squares_settings_s* settings, size_t count, size_t m, float* x,
                                      const float* lower, const float* upper, const float* t, size_t t_stride,
                                      const float* data, mir_least_squares_result_s* results,
                                      const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return mir_optim_amd::launch_batched_bounded<PeakOnBaseline<float>>(settings, count, m, x, lower, upper, t, t_stride, data,
                                                                        results, options, extras);
}
