// batched16_host.h -- host layer of the batched fit for models with 9 to 16 parameters (double; batched16_kernel.h,
// launch_batched16<Model> of include/mir_optim_amd_batched.hpp), shared by the two translation units that hold its extern "C"
// entries: batched16_d.hip (the entries without weights and covariance, with the unweighted k_lm_batched16 instances) and
// batched16_ex_d.hip (the _ex entries and the covariance entry, with the weighted instances and k_batched16_covariance). Two
// units, so that the first compiles the device code it always compiled and the build stays parallel.
#pragma once

#include "batched_host.h"

namespace mirlsq {

// THE dispatch from a MIR_LSQ_MODEL16_* id to the built-in model type: f(Model{}), or -1 for any other id (0, 1 and 2 included:
// those are models of the n <= 8 entries)
template <class F>
int with_builtin_model16(int id, F&& f)
{
    switch (id) {
    case kModel16ExpHarm16: return f(BuiltinModel16<kModel16ExpHarm16>::type{});
    case kModel16Gauss3Affine: return f(BuiltinModel16<kModel16Gauss3Affine>::type{});
    }
    return -1;
}
template <class Model> constexpr int builtin_model16_id()
{
    return std::is_same<Model, BuiltinModel16<kModel16ExpHarm16>::type>::value ? kModel16ExpHarm16 : kModel16Gauss3Affine;
}

// the launch of the UNWEIGHTED fit instance of a built-in model, which batched16_d.hip compiles: false when it could not be made
bool batched16_plain_enqueue(int model, const BatchedArgs<double>& a, size_t lds, hipStream_t stream);

// The host-pointer entry of one model: one allocation, the fit (and, with extras->covariance, the covariance behind it), the
// copies back. extras: HOST pointers, or nullptr. Kernels: the instances the calling unit compiles (launch_batched16_with).
template <class Model, class Kernels>
int batched16_host_model_entry(const mir_least_squares_settings_d* S, size_t count, size_t m, double* x, const double* lower,
                               const double* upper, const double* t, size_t t_stride, const double* data,
                               mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                               const mir_lsq_batched_extras* extras)
{
    using Result = mir_least_squares_result_d;
    constexpr size_t n = Model::n;
    mir_lsq_batched_extras e;
    if (!mir_optim_amd::detail::batched_extras(extras, m, e)) return -1;
    const double* weights = static_cast<const double*>(e.weights);
    double* cov = static_cast<double*>(e.covariance);
    const size_t wn = weights ? (e.weight_stride ? count : 1) * m : 0;
    for (size_t i = 0; i < wn; ++i)
        if (!(-Lim<double>::inf() < weights[i] && weights[i] < Lim<double>::inf())) return -1;   // non-finite weights: the caller's error
    for (size_t i = 0; i < count; ++i) {       // defaults of LeastSquaresResult!T, LS:132-142
        results[i].status = mir_ls_numericError; results[i].iterations = results[i].fCalls = results[i].gCalls = 0;
        results[i].residual = Lim<double>::inf(); results[i].lambda = 0;
    }
    if (count == 0) return 0;
    const int bad = bad_settings(S);           // common to all problems (the code is reported per problem)
    if (!device_available()) return -2;
    if (m == 0 || mir_optim_amd::batched16_lds_bytes<Model>(m) > mir_optim_amd::kBatchedLdsLimit) {
        std::fprintf(stderr, "[mir_optim_amd] batched16 entry: m = %zu does not fit one wave's LDS slice (m <= %zu)\n", m,
                     mir_optim_amd::kBatched16MaxRows);
        return -3;
    }
    if (bad) {
        for (size_t i = 0; i < count; ++i) results[i].status = bad;
        for (size_t i = 0; cov && i < count * n * n; ++i) cov[i] = Lim<double>::inf() - Lim<double>::inf();   // negative status: NaN
        return 0;
    }
    mir_lsq_batched_options o = batched_options(options);
    o.stream = nullptr;
    // one allocation: the arrays, the records, the model's per-row basis table, the weights and the covariance
    const size_t basis_b = mir_optim_amd::batched_basis_floats<Model>(count, m, t_stride) * sizeof(double);
    const size_t tb = (t_stride ? count : 1) * m * sizeof(double), db = count * m * sizeof(double), xb = count * n * sizeof(double);
    const size_t wb = wn * sizeof(double), cb = cov ? count * n * n * sizeof(double) : 0;
    // MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM: lower / upper hold count x n values, row i the box of problem i
    const size_t bb = ((e.flags & MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM) ? count : 1) * n * sizeof(double);
    char* base = nullptr;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o_ = off; off = align_up(off + bytes, 256); return o_; };
    const size_t ot = take(tb), od = take(db), ox = take(xb), ol = take(bb), ou = take(bb),
                 orr = take(count * sizeof(Result)), obasis = take(basis_b), ow = take(wb), oc = take(cb);
    if (hipMalloc((void**)&base, off) != hipSuccess) return -4;
    o.basis = basis_b ? (float*)(base + obasis) : nullptr;      // the C member is float*; it holds doubles here
    o.basis_bytes = basis_b;
    mir_lsq_batched_extras de{};               // the device twin of the extras
    de.struct_size = sizeof de; de.flags = e.flags; de.weights = wb ? base + ow : nullptr; de.weight_stride = e.weight_stride;
    de.covariance = cb ? base + oc : nullptr;
    bool good = hipMemcpy(base + ot, t, tb, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + od, data, db, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ox, x, xb, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ol, lower, bb, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ou, upper, bb, hipMemcpyHostToDevice) == hipSuccess
        && (!wb || hipMemcpy(base + ow, weights, wb, hipMemcpyHostToDevice) == hipSuccess);
    good = good
        && mir_optim_amd::detail::launch_batched16_with<Model, Kernels>(
               S, count, m, (double*)(base + ox), (const double*)(base + ol), (const double*)(base + ou), (const double*)(base + ot),
               t_stride, (const double*)(base + od), (Result*)(base + orr), &o, extras ? &de : nullptr) == 0
        && hipDeviceSynchronize() == hipSuccess
        && hipMemcpy(results, base + orr, count * sizeof(Result), hipMemcpyDeviceToHost) == hipSuccess
        && hipMemcpy(x, base + ox, xb, hipMemcpyDeviceToHost) == hipSuccess
        && (!cb || hipMemcpy(cov, base + oc, cb, hipMemcpyDeviceToHost) == hipSuccess);
    (void)hipFree(base);
    return good ? 0 : -5;
}

}  // namespace mirlsq
