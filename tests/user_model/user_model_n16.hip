// A caller's OWN residual models with 9 to 16 parameters for the batched one-wavefront-per-problem fit
// (include/mir_optim_amd_batched.hpp, launch_batched16<Model>): double, 9 <= n <= 16, x has 16 entries (x[n..16) = 0).
// A family Harm<N>, instantiated at N = 9 and N = 13 -- orders at which the 16-column J^T J tile has padded columns:
//     p0 exp(-t p1) + p2 + sum_{j = 3 .. N - 1} p_j h_j(t),   h_j = sin(k w t) for odd j, cos(k w t) for even j,
//     k = (j - 1) / 2 (integer division), w = pi / 2
// (the formula of the built-in MIR_LSQ_MODEL16_EXP_HARM16 truncated to N parameters), written out here as a user would write
// it, with its own derivative.
// Build (mir_optim_amd/build.py, build_user_model_example): hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I<repo>/include
#include "mir_optim_amd_batched.hpp"

template <int N> struct Harm {
    using value_type = double;
    static constexpr int n = N, nb = N - 3;
    // the harmonics do not depend on the parameters: they are the row's basis values (tabulated once per launch)
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
    // the reference's optional g callback: d eval / d x_j (used with MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN)
    __device__ static void grad(double t, const double* b, const double* x, double* g)
    {
        const double e = exp(-t * x[1]);
        g[0] = e;
        g[1] = -t * x[0] * e;
        g[2] = 1.0;
        for (int j = 3; j < N; ++j) g[j] = b[j - 3];
    }
};

// every pointer is a DEVICE pointer (the contract of mir_lsq_batched16_kernel_d)
extern "C" int user_fit_harm9_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, double* x, const double* lower,
                                const double* upper, const double* t, size_t t_stride, const double* data,
                                mir_least_squares_result_d* results, const mir_lsq_batched_options* options)
{
    return mir_optim_amd::launch_batched16<Harm<9>>(settings, count, m, x, lower, upper, t, t_stride, data, results, options);
}

extern "C" int user_fit_harm13_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, double* x, const double* lower,
                                 const double* upper, const double* t, size_t t_stride, const double* data,
                                 mir_least_squares_result_d* results, const mir_lsq_batched_options* options)
{
    return mir_optim_amd::launch_batched16<Harm<13>>(settings, count, m, x, lower, upper, t, t_stride, data, results, options);
}

// The residual of ONE problem of the built-in 16-parameter model as a device callback of mir_optimize_least_squares_gpu_d
// (flags MIR_LSQ_DEVICE_CALLBACKS): how these fits were run before the batched entry existed, and what
// tests/test_gpu_batched16.py and scripts/batched16.py compare it with.
struct ResidualCtxD { const double* t; const double* data; void* stream; };
__global__ void k_harm16_residual(const double* __restrict__ t, const double* __restrict__ d, const double* __restrict__ x,
                                  double* __restrict__ y, int m)
{
    using Mdl = mirlsq::ModelExpHarm16;
    double p[16], b[Mdl::nb];
    for (int j = 0; j < 16; ++j) p[j] = x[j];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        Mdl::basis(t[i], b);
        y[i] = Mdl::eval(t[i], b, p) - d[i];
    }
}
extern "C" void user_harm16_residual_d(void* ctx, size_t m, size_t n, const double* x, double* y)
{
    (void)n;
    const auto* c = static_cast<const ResidualCtxD*>(ctx);
    hipLaunchKernelGGL(k_harm16_residual, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(c->stream), c->t,
                       c->data, x, y, (int)m);
}
