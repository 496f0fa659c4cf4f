// batched_d.hip -- the batched one-wavefront-per-problem fit in DOUBLE: the f64 instances of launch_batched<Model>
// (include/mir_optim_amd_batched.hpp) for the three built-in models (ModelExpDecayD, ModelExp3AffineD, ModelExpDecayPad8D:
// same ids and formulas as the float ones), the f64 ?posvx unit entry, and the host-pointer entry, which completes problems
// whose step reaches a finite bound with mir_optimize_least_squares_gpu_d. The contract of every entry is its _s twin's
// (batched.hip); this unit is separate so that the fp32 unit and its kernels stay as they are.
#include "driver.h"
#include "launch_util.h"
#include "../../include/mir_optim_amd_batched.hpp"

using namespace mirlsq;

namespace {

inline int batched_model_nb_d(int model)
{
    return model == kModelExpDecay ? ModelExpDecayD::nb : model == kModelExp3Affine ? ModelExp3AffineD::nb : ModelExpDecayPad8D::nb;
}
inline int batched_model_n_d(int model)
{
    return model == kModelExpDecay ? 3 : ((model == kModelExp3Affine || model == kModelExpDecayPad8) ? 8 : 0);
}

int batched_launch_d(int model, const mir_least_squares_settings_d* S, size_t count, size_t m, double* x, const double* lower,
                     const double* upper, const double* t, size_t t_stride, const double* data, mir_least_squares_result_d* results,
                     const mir_lsq_batched_options* opt)
{
    using namespace mir_optim_amd;
    if (model == kModelExpDecay) return launch_batched<ModelExpDecayD>(S, count, m, x, lower, upper, t, t_stride, data, results, opt);
    if (model == kModelExp3Affine) return launch_batched<ModelExp3AffineD>(S, count, m, x, lower, upper, t, t_stride, data, results, opt);
    return launch_batched<ModelExpDecayPad8D>(S, count, m, x, lower, upper, t, t_stride, data, results, opt);
}

struct BatchedFallbackCtxD { const double* t; const double* d; hipStream_t stream; int model; };
void batched_fallback_d(void* vctx, size_t m, size_t n, const double* x, double* y)
{
    (void)n;
    using namespace mir_optim_amd;
    auto* c = static_cast<BatchedFallbackCtxD*>(vctx);
    if (c->model == kModelExpDecay) launch_model_residual<ModelExpDecayD>(c->t, c->d, x, y, m, c->stream);
    else if (c->model == kModelExp3Affine) launch_model_residual<ModelExp3AffineD>(c->t, c->d, x, y, m, c->stream);
    else launch_model_residual<ModelExpDecayPad8D>(c->t, c->d, x, y, m, c->stream);
}

// the options as this build understands them, and the plausibility check of the 0.1 calling convention: as in batched.hip
mir_lsq_batched_options batched_options_d(const mir_lsq_batched_options* opt)
{
    mir_lsq_batched_options o{};
    if (opt) std::memcpy(&o, opt, opt->struct_size < sizeof o ? opt->struct_size : sizeof o);
    o.struct_size = sizeof o;
    return o;
}
bool batched_options_plausible_d(const mir_lsq_batched_options* opt)
{
    return !opt || (opt->struct_size >= 8 && opt->struct_size <= 1024);
}

}  // namespace

extern "C" {

int mir_lsq_batched_kernel_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model, double* x,
                             const double* lower, const double* upper, const double* t, size_t t_stride, const double* data,
                             mir_least_squares_result_d* results, const mir_lsq_batched_options* options)
{
    if (batched_model_n_d(model) == 0 || !batched_options_plausible_d(options)) return -1;
    if (!S || !x || !lower || !upper || !t || !data || !results || (t_stride != 0 && t_stride != m)) return -1;
    if (count != 0 && !device_available()) return -2;
    const mir_lsq_batched_options o = batched_options_d(options);
    return batched_launch_d(model, S, count, m, x, lower, upper, t, t_stride, data, results, &o);
}

int mir_lsq_batched_posvx_d(size_t count, size_t n, const double* P, const double* rhs, double* x, int* info, void* stream)
{
    if (!P || !rhs || !x || !info || (n != 3 && n != 8)) return -1;
    if (count == 0) return 0;
    if (!device_available()) return -2;
    const unsigned blocks = (unsigned)std::min<size_t>(count, 8192);
    if (n == 8)
        hipLaunchKernelGGL((k_posvx_rows<8, double>), dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), P, rhs, (int)count, x, info);
    else
        hipLaunchKernelGGL((k_posvx_rows<3, double>), dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), P, rhs, (int)count, x, info);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int mir_optimize_least_squares_batched_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model,
                                         double* x, const double* lower, const double* upper,
                                         const double* t, size_t t_stride, const double* data,
                                         mir_least_squares_result_d* results, const mir_lsq_batched_options* options)
{
    if (!S || !x || !lower || !upper || !t || !data || !results || !batched_options_plausible_d(options)) return -1;
    const int n = batched_model_n_d(model);
    if (n == 0 || (t_stride != 0 && t_stride != m)) return -1;
    for (size_t i = 0; i < count; ++i) {       // defaults of LeastSquaresResult!T, LS:132-142
        results[i].status = mir_ls_numericError; results[i].iterations = results[i].fCalls = results[i].gCalls = 0;
        results[i].residual = Lim<double>::inf(); results[i].lambda = 0;
    }
    if (count == 0) return 0;
    // settings validation LS:934-943, common to all problems (codes reported per problem)
    int bad = 0;
    if (!(0 <= S->minStepQuality && S->minStepQuality < 1)) bad = mir_ls_badMinStepQuality;
    else if (!(0 <= S->goodStepQuality && S->goodStepQuality <= 1)) bad = mir_ls_badGoodStepQuality;
    else if (!(S->minStepQuality < S->goodStepQuality)) bad = mir_ls_badStepQuality;
    else if (!(1 <= S->lambdaIncrease && S->lambdaIncrease <= std::sqrt(DBL_MAX))) bad = mir_ls_badLambdaParams;
    else if (!(std::sqrt(DBL_MIN) <= S->lambdaDecrease && S->lambdaDecrease <= 1)) bad = mir_ls_badLambdaParams;
    if (!device_available()) return -2;
    const size_t lds = (size_t)(n + 2) * m * sizeof(double);
    if (m == 0 || lds > mir_optim_amd::kBatchedLdsLimit) {
        std::fprintf(stderr, "[mir_optim_amd] batched f64 entry: m = %zu does not fit one wave's LDS slice\n", m);
        return -3;
    }
    mir_lsq_batched_options o = batched_options_d(options);
    o.stream = nullptr;
    // the model's per-row basis table (doubles) is part of this call's one allocation
    const size_t basis_b = (t_stride ? count : 1) * m * (size_t)batched_model_nb_d(model) * sizeof(double);
    const size_t tb = (t_stride ? count : 1) * m * sizeof(double), db = count * m * sizeof(double), xb = count * n * sizeof(double);
    char* base = nullptr;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o_ = off; off = align_up(off + bytes, 256); return o_; };
    const size_t ot = take(tb), od = take(db), ox = take(xb), ol = take(n * sizeof(double)), ou = take(n * sizeof(double)),
                 orr = take(count * sizeof(BatchedResult<double>)), obasis = take(basis_b);
    if (hipMalloc((void**)&base, off) != hipSuccess) return -4;
    o.basis = basis_b ? (float*)(base + obasis) : nullptr;      // the C member is float*; it holds doubles for a double model
    o.basis_bytes = basis_b;
    bool good = hipMemcpy(base + ot, t, tb, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + od, data, db, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ox, x, xb, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ol, lower, n * sizeof(double), hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ou, upper, n * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    const double* dt = (const double*)(base + ot); const double* ddata = (const double*)(base + od); double* dx = (double*)(base + ox);
    const double* dlower = (const double*)(base + ol); const double* dupper = (const double*)(base + ou);
    mir_least_squares_result_d* dres = (mir_least_squares_result_d*)(base + orr);
    std::vector<BatchedResult<double>> res(count);
    std::vector<double> x0(x, x + count * n);      // starts, for the fallback problems
    if (good && !bad) {
        good = batched_launch_d(model, S, count, m, dx, dlower, dupper, dt, t_stride, ddata, dres, &o) == 0;
        good = good && hipDeviceSynchronize() == hipSuccess
            && hipMemcpy(res.data(), dres, count * sizeof(BatchedResult<double>), hipMemcpyDeviceToHost) == hipSuccess
            && hipMemcpy(x, dx, xb, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (good) {
        for (size_t i = 0; i < count; ++i) {
            if (bad) { results[i].status = bad; continue; }
            results[i].status = res[i].status; results[i].iterations = res[i].iterations; results[i].fCalls = res[i].fCalls;
            results[i].gCalls = res[i].gCalls; results[i].residual = res[i].residual; results[i].lambda = res[i].lambda;
            if (res[i].status == kBatchedNeedsGeneral) {
                // bounded step: complete this problem with the general solver (device callbacks, BOXCQP on the device)
                hipStream_t st = nullptr;
                if (hipStreamCreate(&st) != hipSuccess) { good = false; break; }
                BatchedFallbackCtxD c{dt + (t_stride ? i * m : 0), ddata + i * m, st, model};
                mir_lsq_gpu_options go{};
                go.struct_size = sizeof go; go.flags = MIR_LSQ_DEVICE_CALLBACKS; go.stream = st;
                std::memcpy(x + i * n, x0.data() + i * n, n * sizeof(double));
                results[i] = mir_optimize_least_squares_gpu_d(S, m, n, x + i * n, lower, upper, &go, &c, batched_fallback_d,
                                                              nullptr, nullptr, nullptr, nullptr);
                (void)hipStreamDestroy(st);
            }
        }
    }
    (void)hipFree(base);
    return good ? 0 : -5;
}

}  // extern "C"
