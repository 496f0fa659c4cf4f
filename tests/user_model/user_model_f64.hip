// A caller's OWN residual model in DOUBLE for the batched one-wavefront-per-problem fit (include/mir_optim_amd_batched.hpp):
// `using value_type = double;` makes launch_batched<Model> take the _d settings and result records and double arrays, as
// mir_lsq_batched_kernel_d does. Five parameters (not one of the built-in orders 3 and 8) and its own derivative.
// Build (mir_optim_amd/build.py, build_user_model_example): hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I<repo>/include
#include "mir_optim_amd_batched.hpp"

// damped oscillation on a baseline: p0 exp(-p1 t) cos(p2 t) + p3 + p4 sqrt(t)      (n = 5)
// sqrt(t) does not depend on the parameters: it is the row's basis value (tabulated once per launch, in double)
struct DampedCosineD {
    using value_type = double;
    static constexpr int n = 5, nb = 1;
    __device__ static void basis(double t, double* b) { b[0] = sqrt(t); }
    __device__ static double eval(double t, const double* b, const double* x)
    {
        return x[0] * exp(-x[1] * t) * cos(x[2] * t) + x[3] + x[4] * b[0];
    }
    // the reference's optional g callback: d eval / d x_j (used with MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN)
    __device__ static void grad(double t, const double* b, const double* x, double* g)
    {
        const double e = exp(-x[1] * t), c = cos(x[2] * t), s = sin(x[2] * t);
        g[0] = e * c;
        g[1] = -t * x[0] * e * c;
        g[2] = -t * x[0] * e * s;
        g[3] = 1.0;
        g[4] = b[0];
    }
};

// every pointer is a DEVICE pointer (the contract of mir_lsq_batched_kernel_d)
extern "C" int user_fit_damped_cosine_d(const mir_least_squares_settings_d* settings, size_t count, size_t m, double* x,
                                        const double* lower, const double* upper, const double* t, size_t t_stride,
                                        const double* data, mir_least_squares_result_d* results,
                                        const mir_lsq_batched_options* options)
{
    return mir_optim_amd::launch_batched<DampedCosineD>(settings, count, m, x, lower, upper, t, t_stride, data, results, options);
}

// The residual of ONE problem as a device callback of mir_optimize_least_squares_gpu_d (flags MIR_LSQ_DEVICE_CALLBACKS): the
// double form of launch_model_residual<Model>, here for the built-in double model of MIR_LSQ_MODEL_EXP_DECAY_PAD8 -- how a
// caller completes a problem that came back from the kernel entry with status -100, and what tests/test_gpu_batched_f64.py
// compares the batched fit with.
struct ResidualCtxD { const double* t; const double* data; void* stream; };
extern "C" void user_pad8_residual_d(void* ctx, size_t m, size_t n, const double* x, double* y)
{
    (void)n;
    const auto* c = static_cast<const ResidualCtxD*>(ctx);
    mir_optim_amd::launch_model_residual<mirlsq::ModelExpDecayPad8D>(c->t, c->data, x, y, m, static_cast<hipStream_t>(c->stream));
}
