// A caller's OWN residual model fitted under BOX CONSTRAINTS THAT BIND, through the public device header alone
// (include/mir_optim_amd_batched.hpp): launch_batched_bounded<Model> runs the bounded instance of the model's kernel, which
// solves the box QP of a step that leaves the box inside the kernel -- one launch finishes every problem, none returns -100.
// The last entry hands the same model to launch_batched<Model>, which does not hold that instance: with
// MIR_LSQ_BATCHED_DEVICE_BOUNDS in the options it answers -1.
// Build (mir_optim_amd/build.py, user_model_bounded_lib): hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I<repo>/include
#include "mir_optim_amd_batched.hpp"

// logistic growth on a background: p0 / (1 + exp(-p1 (t - p2))) + p3      (n = 4)
// a caller who knows the capacity of the medium passes upper[0] = that capacity
template <class T> struct LogisticGrowth {
    using value_type = T;
    static constexpr int n = 4, nb = 0;
    __device__ static void basis(T, T*) {}
    __device__ static T eval(T t, const T*, const T* x) { return x[0] / (T(1) + exp(-x[1] * (t - x[2]))) + x[3]; }
};

// every pointer is a DEVICE pointer (the contract of mir_lsq_batched_kernel_s / _d)
extern "C" int user_fit_logistic_bounded_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, double* x,
                                           const double* lower, const double* upper, const double* t, size_t t_stride,
                                           const double* data, mir_least_squares_result_d* results,
                                           const mir_lsq_batched_options* options)
{
    return mir_optim_amd::launch_batched_bounded<LogisticGrowth<double>>(settings, count, m, x, lower, upper, t, t_stride, data,
                                                                         results, options);
}
extern "C" int user_fit_logistic_bounded_s(const mir_least_squares_settings_s* settings, size_t count, size_t m, float* x,
                                           const float* lower, const float* upper, const float* t, size_t t_stride,
                                           const float* data, mir_least_squares_result_s* results,
                                           const mir_lsq_batched_options* options)
{
    return mir_optim_amd::launch_batched_bounded<LogisticGrowth<float>>(settings, count, m, x, lower, upper, t, t_stride, data,
                                                                        results, options);
}

// the default instance of the same model: status -100 for a problem whose step reaches a bound
extern "C" int user_fit_logistic_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, double* x,
                                   const double* lower, const double* upper, const double* t, size_t t_stride, const double* data,
                                   mir_least_squares_result_d* results, const mir_lsq_batched_options* options)
{
    return mir_optim_amd::launch_batched<LogisticGrowth<double>>(settings, count, m, x, lower, upper, t, t_stride, data, results,
                                                                 options);
}
