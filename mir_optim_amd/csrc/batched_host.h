// batched_host.h -- host layer of the batched path (BASELINE cfg 5: many small independent fits, one wavefront per problem,
// batched_kernel.h), written once in the value type T. The launch itself is the public device-header template
// launch_batched<Model> (include/mir_optim_amd_batched.hpp); this header adds, for the three compiled-in models of T,
//   batched_kernel_entry<T>   the device-pointer entry (mir_lsq_batched_kernel_s / _d and, with extras, _ex_s / _ex_d),
//   batched_covariance_entry<T>  the covariance kernel on its own (mir_lsq_batched_covariance_s / _d),
//   batched_posvx_entry<T>    the ?posvx unit entry (mir_lsq_batched_posvx_s / _d),
//   batched_host_entry<T>     the host-pointer entry (mir_optimize_least_squares_batched_s / _d), which completes problems whose
//                             step reaches a finite bound with the general solver (BOXCQP on the device, boxcqp.d:234-376) --
//                             with MIR_LSQ_BATCHED_DEVICE_BOUNDS the kernel finishes them and that loop finds nothing to do.
// batched.hip (float) and batched_d.hip (double) instantiate one precision each -- two translation units, so that the six
// k_lm_batched instances compile in parallel -- and hold that precision's extern "C" forwarders.
// Nothing here is process-wide state: the A/B switch of the ladder and the profiling buffer travel in mir_lsq_batched_options.
#pragma once

#include "driver.h"
#include "../../include/mir_optim_amd_batched.hpp"

namespace mirlsq {

// THE dispatch from a MIR_LSQ_MODEL_* id and T to the built-in model type: f(Model{}), or -1 for an unknown id
template <class T, class F>
int with_builtin_model(int id, F&& f)
{
    switch (id) {
    case kModelExpDecay: return f(typename BuiltinModel<kModelExpDecay, T>::type{});
    case kModelExp3Affine: return f(typename BuiltinModel<kModelExp3Affine, T>::type{});
    case kModelExpDecayPad8: return f(typename BuiltinModel<kModelExpDecayPad8, T>::type{});
    }
    return -1;
}

// The BOUNDED kernel instances of the three built-in models (k_lm_batched<Model, WEIGHTED, BatchedBoxQpStep>, batched_bounded.h)
// are compiled in translation units of their own -- batched_bounded.hip (float), batched_bounded_d.hip (double) -- so that
// batched.hip / batched_d.hip compile the device code they always compiled and the build stays parallel. This is their launch:
// false when it could not be made.
bool batched_bounded_enqueue(int model, const BatchedArgs<float>& a, bool weighted, size_t lds, hipStream_t stream);
bool batched_bounded_enqueue(int model, const BatchedArgs<double>& a, bool weighted, size_t lds, hipStream_t stream);
// what the two units define it with
template <class T>
bool batched_bounded_enqueue_builtin(int model, const BatchedArgs<T>& a, bool weighted, size_t lds, hipStream_t stream)
{
    return with_builtin_model<T>(model, [&](auto mdl) {
        return (int)mir_optim_amd::detail::enqueue_fit<decltype(mdl), BatchedBoxQpStep>(a, weighted, lds, stream);
    }) == 1;
}

template <class Model> constexpr int builtin_model_id()
{
    using T = batched_value_t<Model>;
    return std::is_same<Model, typename BuiltinModel<kModelExpDecay, T>::type>::value ? kModelExpDecay
        : std::is_same<Model, typename BuiltinModel<kModelExp3Affine, T>::type>::value ? kModelExp3Affine : kModelExpDecayPad8;
}

// launch_batched<Model> for a built-in model as the C entries make it: the default instances of this unit, or -- with
// MIR_LSQ_BATCHED_DEVICE_BOUNDS in the options -- the bounded ones of the other unit
template <class Model, class T = batched_value_t<Model>>
int launch_builtin(const typename Abi<T>::Settings* S, size_t count, size_t m, T* x, const T* lower, const T* upper, const T* t,
                   size_t t_stride, const T* data, typename Abi<T>::Result* results, const mir_lsq_batched_options* o,
                   const mir_lsq_batched_extras* extras)
{
    if (!(o && (o->variant & MIR_LSQ_BATCHED_DEVICE_BOUNDS)))
        return mir_optim_amd::launch_batched<Model>(S, count, m, x, lower, upper, t, t_stride, data, results, o, extras);
    return mir_optim_amd::detail::launch_batched_with<Model>(
        S, count, m, x, lower, upper, t, t_stride, data, results, o, extras,
        [](const BatchedArgs<T>& a, bool weighted, size_t lds, hipStream_t stream) {
            return batched_bounded_enqueue(builtin_model_id<Model>(), a, weighted, lds, stream);
        });
}

// the options as this build understands them (struct_size-versioned like mir_lsq_gpu_options)
inline mir_lsq_batched_options batched_options(const mir_lsq_batched_options* opt)
{
    mir_lsq_batched_options o{};
    if (opt) std::memcpy(&o, opt, opt->struct_size < sizeof o ? opt->struct_size : sizeof o);
    o.struct_size = sizeof o;
    return o;
}
// A caller of the 0.1 interface passed a hipStream_t where the options pointer is now (same arity: it links). Its first word is
// not a struct size: anything below the two leading members or absurdly large is refused instead of being copied from.
inline bool batched_options_plausible(const mir_lsq_batched_options* opt)
{
    return !opt || (opt->struct_size >= 8 && opt->struct_size <= 1024);
}

// the extras (weights, covariance) are plausible: a struct size, and a weight_stride of 0 or m. NULL = none.
inline bool batched_extras_plausible(const mir_lsq_batched_extras* extras, size_t m)
{
    mir_lsq_batched_extras e;
    return mir_optim_amd::detail::batched_extras(extras, m, e);
}

// Both precisions check in one order: model id, options and extras, then pointers and t_stride (-1), then the device (-2).
template <class T>
int batched_kernel_entry(const typename Abi<T>::Settings* S, size_t count, size_t m, int model, T* x, const T* lower, const T* upper,
                         const T* t, size_t t_stride, const T* data, typename Abi<T>::Result* results,
                         const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras = nullptr)
{
    return with_builtin_model<T>(model, [&](auto mdl) {
        if (!batched_options_plausible(options) || !batched_extras_plausible(extras, m)) return -1;
        if (!S || !x || !lower || !upper || !t || !data || !results || (t_stride != 0 && t_stride != m)) return -1;
        if (count != 0 && !device_available()) return -2;
        const mir_lsq_batched_options o = batched_options(options);
        return launch_builtin<decltype(mdl)>(S, count, m, x, lower, upper, t, t_stride, data, results, &o, extras);
    });
}

template <class T>
int batched_covariance_entry(const typename Abi<T>::Settings* S, size_t count, size_t m, int model, const T* x, const T* lower,
                             const T* upper, const T* t, size_t t_stride, const T* data, const typename Abi<T>::Result* results,
                             const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return with_builtin_model<T>(model, [&](auto mdl) {
        mir_lsq_batched_extras e;
        if (!batched_options_plausible(options) || !extras || !mir_optim_amd::detail::batched_extras(extras, m, e) || !e.covariance)
            return -1;
        if (!S || !x || !lower || !upper || !t || !data || !results || (t_stride != 0 && t_stride != m)) return -1;
        if (count != 0 && !device_available()) return -2;
        const mir_lsq_batched_options o = batched_options(options);
        return mir_optim_amd::launch_batched_covariance<decltype(mdl)>(S, count, m, x, lower, upper, t, t_stride, data, results, &o, extras);
    });
}

template <class T>
int batched_posvx_entry(size_t count, size_t n, const T* P, const T* rhs, T* x, int* info, void* stream)
{
    if (!P || !rhs || !x || !info || (n != 3 && n != 8)) return -1;
    if (count == 0) return 0;
    if (!device_available()) return -2;
    const unsigned blocks = (unsigned)std::min<size_t>(count, 8192);
    if (n == 8) hipLaunchKernelGGL((k_posvx_rows<8, T>), dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), P, rhs, (int)count, x, info);
    else hipLaunchKernelGGL((k_posvx_rows<3, T>), dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), P, rhs, (int)count, x, info);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

// the general solver's device callback for ONE problem of the batch: its residual vector by the model's own kernel
template <class T> struct BatchedFallbackCtx { const T* t; const T* d; hipStream_t stream; const T* w; };   // w: the problem's weights or nullptr
template <class Model>
void batched_fallback(void* vctx, size_t m, size_t, const batched_value_t<Model>* x, batched_value_t<Model>* y)
{
    auto* c = static_cast<BatchedFallbackCtx<batched_value_t<Model>>*>(vctx);
    mir_optim_amd::launch_model_residual<Model>(c->t, c->d, x, y, m, c->stream, c->w);
}

template <class Model, class T = batched_value_t<Model>>
int batched_host_model_entry(const typename Abi<T>::Settings* S, size_t count, size_t m, T* x, const T* lower, const T* upper,
                             const T* t, size_t t_stride, const T* data, typename Abi<T>::Result* results,
                             const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    using Result = typename Abi<T>::Result;
    constexpr size_t n = Model::n;
    mir_lsq_batched_extras e;                  // HOST pointers here
    if (!batched_options_plausible(options) || !mir_optim_amd::detail::batched_extras(extras, m, e)) return -1;
    const T* weights = static_cast<const T*>(e.weights);
    T* cov = static_cast<T*>(e.covariance);
    const size_t wn = weights ? (e.weight_stride ? count : 1) * m : 0;
    for (size_t i = 0; i < wn; ++i)
        if (!(-Lim<T>::inf() < weights[i] && weights[i] < Lim<T>::inf())) return -1;      // non-finite weights: the caller's error
    if (!S || !x || !lower || !upper || !t || !data || !results) return -1;
    if (t_stride != 0 && t_stride != m) return -1;
    for (size_t i = 0; i < count; ++i) {       // defaults of LeastSquaresResult!T, LS:132-142
        results[i].status = mir_ls_numericError; results[i].iterations = results[i].fCalls = results[i].gCalls = 0;
        results[i].residual = Lim<T>::inf(); results[i].lambda = 0;
    }
    if (count == 0) return 0;
    const int bad = bad_settings(S);           // common to all problems (the code is reported per problem)
    if (!device_available()) return -2;
    if (m == 0 || mir_optim_amd::batched_lds_bytes<Model>(m) > mir_optim_amd::kBatchedLdsLimit) {
        std::fprintf(stderr, "[mir_optim_amd] batched %sentry: m = %zu does not fit one wave's LDS slice\n",
                     std::is_same<T, double>::value ? "f64 " : "", m);
        return -3;
    }
    mir_lsq_batched_options o = batched_options(options);
    o.stream = nullptr;
    // the model's per-row basis table (values of T) is part of this call's one allocation
    const size_t basis_b = mir_optim_amd::batched_basis_floats<Model>(count, m, t_stride) * sizeof(T);
    const size_t tb = (t_stride ? count : 1) * m * sizeof(T), db = count * m * sizeof(T), xb = count * n * sizeof(T);
    char* base = nullptr;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o_ = off; off = align_up(off + bytes, 256); return o_; };
    const size_t wb = wn * sizeof(T), cb = cov ? count * n * n * sizeof(T) : 0;
    // MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM: lower / upper hold count x n values, row i the box of problem i
    const size_t bstep = (e.flags & MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM) ? n : 0, bb = (bstep ? count : 1) * n * sizeof(T);
    const size_t ot = take(tb), od = take(db), ox = take(xb), ol = take(bb), ou = take(bb),
                 orr = take(count * sizeof(Result)), obasis = take(basis_b), ow = take(wb), oc = take(cb);
    if (hipMalloc((void**)&base, off) != hipSuccess) return -4;
    o.basis = basis_b ? (float*)(base + obasis) : nullptr;      // the C member is float*; it holds doubles for a double model
    o.basis_bytes = basis_b;
    bool good = hipMemcpy(base + ot, t, tb, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + od, data, db, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ox, x, xb, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ol, lower, bb, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ou, upper, bb, hipMemcpyHostToDevice) == hipSuccess
        && (!wb || hipMemcpy(base + ow, weights, wb, hipMemcpyHostToDevice) == hipSuccess);
    // the device twin of the extras: the weights for the fit; the covariance comes after the fallback solves, below
    const T* dw = wb ? (const T*)(base + ow) : nullptr;
    mir_lsq_batched_extras de{};
    de.struct_size = sizeof de; de.flags = e.flags; de.weights = dw; de.weight_stride = e.weight_stride;
    const T* dt = (const T*)(base + ot); const T* ddata = (const T*)(base + od); T* dx = (T*)(base + ox);
    Result* dres = (Result*)(base + orr);      // the kernel writes the C records in place (launch_batched asserts the layout)
    std::vector<Result> res(count);
    std::vector<T> x0(x, x + count * n);       // starts, for the fallback problems
    if (good && !bad) {
        good = launch_builtin<Model>(S, count, m, dx, (const T*)(base + ol), (const T*)(base + ou), dt, t_stride, ddata, dres, &o,
                                     extras ? &de : nullptr) == 0;
        good = good && hipDeviceSynchronize() == hipSuccess
            && hipMemcpy(res.data(), dres, count * sizeof(Result), hipMemcpyDeviceToHost) == hipSuccess
            && hipMemcpy(x, dx, xb, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (good) {
        for (size_t i = 0; i < count; ++i) {
            if (bad) { results[i].status = bad; continue; }
            results[i] = res[i];
            if (res[i].status == kBatchedNeedsGeneral) {
                // bounded step: complete this problem with the general solver (device callbacks, BOXCQP on the device) --
                // solve_entry<T> is all there is to mir_optimize_least_squares_gpu_s / _d
                hipStream_t st = nullptr;
                if (hipStreamCreate(&st) != hipSuccess) { good = false; break; }
                BatchedFallbackCtx<T> c{dt + (t_stride ? i * m : 0), ddata + i * m, st, dw ? dw + (e.weight_stride ? i * m : 0) : nullptr};
                mir_lsq_gpu_options go{};
                go.struct_size = sizeof go; go.flags = MIR_LSQ_DEVICE_CALLBACKS; go.stream = st;
                std::memcpy(x + i * n, x0.data() + i * n, n * sizeof(T));
                results[i] = solve_entry<T>(S, m, n, x + i * n, lower + i * bstep, upper + i * bstep, &go, &c, batched_fallback<Model>, nullptr, nullptr,
                                            nullptr, nullptr);
                (void)hipStreamDestroy(st);
            }
        }
    }
    if (good && cov && bad) {
        for (size_t i = 0; i < count * n * n; ++i) cov[i] = Lim<T>::inf() - Lim<T>::inf();     // negative status: NaN
    } else if (good && cov) {
        // the covariance at every problem's FINAL x: the records and x of the fallback problems go back to the device first
        de.covariance = base + oc;
        good = hipMemcpy(dres, results, count * sizeof(Result), hipMemcpyHostToDevice) == hipSuccess
            && hipMemcpy(dx, x, xb, hipMemcpyHostToDevice) == hipSuccess
            && mir_optim_amd::launch_batched_covariance<Model>(S, count, m, dx, (const T*)(base + ol), (const T*)(base + ou), dt,
                                                               t_stride, ddata, dres, &o, &de) == 0
            && hipDeviceSynchronize() == hipSuccess
            && hipMemcpy(cov, base + oc, cb, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(base);
    return good ? 0 : -5;
}

template <class T>
int batched_host_entry(const typename Abi<T>::Settings* S, size_t count, size_t m, int model, T* x, const T* lower, const T* upper,
                       const T* t, size_t t_stride, const T* data, typename Abi<T>::Result* results,
                       const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras = nullptr)
{
    return with_builtin_model<T>(model, [&](auto mdl) {
        return batched_host_model_entry<decltype(mdl)>(S, count, m, x, lower, upper, t, t_stride, data, results, options, extras);
    });
}

}  // namespace mirlsq
