// The FITTED CURVE and its 1-sigma CONFIDENCE BAND for a caller's OWN models, through the public device header alone
// (include/mir_optim_amd_batched.hpp): launch_batched_predict<Model> on the x and the covariance that launch_batched<Model> /
// launch_batched16<Model> with a mir_lsq_batched_extras left on the device (user_model_weighted.hip, user_model_n16_weighted.hip:
// the models of those two examples, restated here). One template serves both widths: a 5-parameter model in float and in
// double, and a 13-parameter model in double. Both have their own derivative, so the band can be formed with it
// (MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN) or with the central differences that built the covariance.
// Build (mir_optim_amd/build.py, user_model_predict_lib): hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I<repo>/include
#include "mir_optim_amd_batched.hpp"

// a peak on a sloping baseline: p0 exp(-(t - p1)^2 / (2 p2^2)) + p3 + p4 t      (n = 5)
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

// p0 exp(-t p1) + p2 + sum_{j = 3 .. N - 1} p_j h_j(t),   h_j = sin(k w t) for odd j, cos(k w t) for even j,
// k = (j - 1) / 2 (integer division), w = pi / 2
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

// every pointer is a DEVICE pointer (the contract of mir_lsq_batched_predict_s / _d); sigma may be NULL, covariance then too
#define USER_PREDICT_ENTRY(NAME, MODEL, T, SETTINGS)                                                                                  \
    extern "C" int NAME(const SETTINGS* settings, size_t count, size_t q, const T* x, const T* lower, const T* upper, const T* tq,     \
                        size_t tq_stride, const T* covariance, T* value, T* sigma, const mir_lsq_batched_options* options,            \
                        const mir_lsq_batched_extras* extras)                                                                         \
    {                                                                                                                                 \
        return mir_optim_amd::launch_batched_predict<MODEL>(settings, count, q, x, lower, upper, tq, tq_stride, covariance, value,    \
                                                            sigma, options, extras);                                                  \
    }

USER_PREDICT_ENTRY(user_predict_peak_s, WeightedPeak<float>, float, mir_least_squares_settings_s)
USER_PREDICT_ENTRY(user_predict_peak_d, WeightedPeak<double>, double, mir_least_squares_settings_d)
USER_PREDICT_ENTRY(user_predict_harm13_d, Harm<13>, double, mir_least_squares_settings_d)
