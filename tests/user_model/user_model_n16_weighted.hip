// A caller's OWN residual models with 9 and 13 parameters fitted with PER-ROW WEIGHTS, and the COVARIANCE of their fitted
// parameters, through the public device header alone (include/mir_optim_amd_batched.hpp): launch_batched16<Model> with a
// mir_lsq_batched_extras, and launch_batched16_covariance<Model> on the records of an earlier launch. The family is the Harm<N>
// of user_model_n16.hip (orders at which the 16-column J^T J tile has padded columns), with its own derivative, so both
// Jacobians (MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN and central differences) are exercised:
//     p0 exp(-t p1) + p2 + sum_{j = 3 .. N - 1} p_j h_j(t),   h_j = sin(k w t) for odd j, cos(k w t) for even j,
//     k = (j - 1) / 2 (integer division), w = pi / 2
// Build (mir_optim_amd/build.py, user_model_n16_weighted_lib): hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I<repo>/include
#include "mir_optim_amd_batched.hpp"

template <int N> struct Harm {
    using value_type = double;
    static constexpr int n = N, nb = N - 3;
    __device__ static void basis(double t, double* b)
    {
        const double w = 1.5707963267948966;
        for (int j = 3; j < N; ++j) {
            const int k = (j - 1) / 2;
            b[j - 3] = (j % 2) ? sin(k * w * t) : cos(k * w * t);
        }
    }
    __device__ static double eval(double t, const double* b, const double* x)
    {
        double v = x[0] * exp(-t * x[1]) + x[2];
        for (int j = 3; j < N; ++j) v += x[j] * b[j - 3];
        return v;
    }
    __device__ static void grad(double t, const double* b, const double* x, double* g)
    {
        const double e = exp(-t * x[1]);
        g[0] = e;
        g[1] = -t * x[0] * e;
        g[2] = 1.0;
        for (int j = 3; j < N; ++j) g[j] = b[j - 3];
    }
};

// every pointer, those in `extras` included, is a DEVICE pointer (the contract of mir_lsq_batched16_kernel_ex_d)
#define USER_HARM_ENTRIES(N)                                                                                                          \
    extern "C" int user_fit_weighted_harm##N##_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, double* x,        \
                                                 const double* lower, const double* upper, const double* t, size_t t_stride,            \
                                                 const double* data, mir_least_squares_result_d* results,                               \
                                                 const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)         \
    {                                                                                                                                 \
        return mir_optim_amd::launch_batched16<Harm<N>>(settings, count, m, x, lower, upper, t, t_stride, data, results, options,       \
                                                        extras);                                                                      \
    }                                                                                                                                 \
    /* the covariance alone, from the x and the records a fit left on the device */                                                   \
    extern "C" int user_weighted_harm##N##_covariance_d(const mir_least_squares_settings_d* settings, size_t count, size_t m,           \
                                                        const double* x, const double* lower, const double* upper, const double* t,    \
                                                        size_t t_stride, const double* data,                                           \
                                                        const mir_least_squares_result_d* results,                                     \
                                                        const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)  \
    {                                                                                                                                 \
        return mir_optim_amd::launch_batched16_covariance<Harm<N>>(settings, count, m, x, lower, upper, t, t_stride, data, results,     \
                                                                   options, extras);                                                  \
    }

USER_HARM_ENTRIES(9)
USER_HARM_ENTRIES(13)
