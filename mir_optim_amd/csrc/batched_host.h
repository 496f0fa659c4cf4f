// batched_host.h -- host layer of the batched path (BASELINE cfg 5: many small independent fits, one wavefront per problem,
// batched_kernel.h; models of 9 to 16 parameters: batched16_kernel.h), written once for both kernel families and both value
// types. The launch itself is the public device header's (include/mir_optim_amd_batched.hpp: detail::launch_fit_with,
// detail::launch_covariance_with); this header adds, for the compiled-in models of a group `Models` (BuiltinModels<T>: the three
// MIR_LSQ_MODEL_* of T; BuiltinModels16<...>: the two MIR_LSQ_MODEL16_*, double),
//   batched_kernel_entry<Models>   the device-pointer entries (mir_lsq_batched_kernel_s / _d, _ex_s / _ex_d, mir_lsq_batched16_kernel_d / _ex_d),
//   batched_covariance_entry<Models>  the covariance kernel on its own (mir_lsq_batched_covariance_s / _d, mir_lsq_batched16_covariance_d),
//   batched_host_entry<Models>     the host-pointer entries (mir_optimize_least_squares_batched_s / _d, _ex_s / _ex_d, ..._batched16_d /
//                                  _ex_d); for n <= 8 they complete problems whose step reaches a finite bound with the general solver
//                                  (BOXCQP on the device, boxcqp.d:234-376) -- with MIR_LSQ_BATCHED_DEVICE_BOUNDS the kernel finishes
//                                  them and that loop finds nothing to do,
//   batched_posvx_entry<T>         the ?posvx unit entry (mir_lsq_batched_posvx_s / _d).
// batched.hip (float), batched_d.hip (double), batched16_d.hip and batched16_ex_d.hip hold the extern "C" forwarders and, with
// batched_bounded.hip / batched_bounded_d.hip, instantiate the kernels -- six translation units, which compile in parallel.
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

// ... and from a MIR_LSQ_MODEL16_* id to the built-in model of 9 to 16 parameters (double): -1 for any other id, 0, 1 and 2 included
template <class F>
int with_builtin_model16(int id, F&& f)
{
    switch (id) {
    case kModel16ExpHarm16: return f(BuiltinModel16<kModel16ExpHarm16>::type{});
    case kModel16Gauss3Affine: return f(BuiltinModel16<kModel16Gauss3Affine>::type{});
    }
    return -1;
}

template <class Model> constexpr int builtin_model_id()
{
    using T = batched_value_t<Model>;
    return std::is_same<Model, typename BuiltinModel<kModelExpDecay, T>::type>::value ? kModelExpDecay
        : std::is_same<Model, typename BuiltinModel<kModelExp3Affine, T>::type>::value ? kModelExp3Affine : kModelExpDecayPad8;
}
template <class Model> constexpr int builtin_model16_id()
{
    return std::is_same<Model, BuiltinModel16<kModel16ExpHarm16>::type>::value ? kModel16ExpHarm16 : kModel16Gauss3Affine;
}

// Each translation unit of the batched path compiles the kernel instances it always compiled, so that the build stays parallel;
// a launch takes them from a `Kernels` policy (include/mir_optim_amd_batched.hpp), and the policy of a unit forwards what the
// unit does not compile to the unit that does, through these functions (false: the launch could not be made):
// the BOUNDED instances of the n <= 8 models (k_lm_batched<Model, WEIGHTED, BatchedBoxQpStep>, batched_bounded.h) are in
// batched_bounded.hip (float) and batched_bounded_d.hip (double),
bool batched_bounded_enqueue(int model, const BatchedArgs<float>& a, bool weighted, size_t lds, hipStream_t stream);
bool batched_bounded_enqueue(int model, const BatchedArgs<double>& a, bool weighted, size_t lds, hipStream_t stream);
// (what the two units define it with)
template <class T>
bool batched_bounded_enqueue_builtin(int model, const BatchedArgs<T>& a, bool weighted, size_t lds, hipStream_t stream)
{
    return with_builtin_model<T>(model, [&](auto mdl) {
        return (int)mir_optim_amd::detail::BatchedKernels<decltype(mdl), BatchedBoxQpStep>::fit(a, weighted, lds, stream);
    }) == 1;
}
// and the UNWEIGHTED fit instances of the 9 to 16 parameter models are in batched16_d.hip.
bool batched16_plain_enqueue(int model, const BatchedArgs<double>& a, size_t lds, hipStream_t stream);

// The kernels of a built-in n <= 8 model as batched.hip / batched_d.hip launch them: the default instances of the unit, or --
// with MIR_LSQ_BATCHED_DEVICE_BOUNDS in the options -- the bounded ones of the other unit
template <class Model> struct BuiltinKernels {
    using T = batched_value_t<Model>;
    using Default = mir_optim_amd::detail::BatchedKernels<Model, BatchedNoBoundedStep>;
    static bool fit(const BatchedArgs<T>& a, bool weighted, size_t lds, hipStream_t stream)
    {
        if (a.variant & MIR_LSQ_BATCHED_DEVICE_BOUNDS) return batched_bounded_enqueue(builtin_model_id<Model>(), a, weighted, lds, stream);
        return Default::fit(a, weighted, lds, stream);
    }
    static bool covariance(const BatchedCovArgs<T>& c, size_t lds, hipStream_t stream) { return Default::covariance(c, lds, stream); }
};

// What the extern "C" entries of one group share, as the `Models` parameter of the entry templates below: the value type, the
// dispatch from the model id, the kernels of a model, and two rules.
//   kPlain: the entry takes neither weights nor covariance (-1; they have entries of their own) and hands on the
//           per-problem-bounds bit of its extras and nothing else;
//   kRefusesAnalytic: MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN for a model without grad is answered -1 with the argument checks (the
//           n <= 8 entries leave it to the launch: none of their models has grad, and the answer comes after the device check).
template <class T> struct BuiltinModels {                           // MIR_LSQ_MODEL_*: batched.hip, batched_d.hip
    using value_type = T;
    template <class Model> using Kernels = BuiltinKernels<Model>;
    static constexpr bool kPlain = false, kRefusesAnalytic = false;
    template <class F> static int with_model(int id, F&& f) { return with_builtin_model<T>(id, f); }
};
template <template <class> class KernelsOf, bool kPlainEntry> struct BuiltinModels16 {      // MIR_LSQ_MODEL16_*: batched16_d.hip, batched16_ex_d.hip
    using value_type = double;
    template <class Model> using Kernels = KernelsOf<Model>;
    static constexpr bool kPlain = kPlainEntry, kRefusesAnalytic = true;
    template <class F> static int with_model(int id, F&& f) { return with_builtin_model16(id, f); }
};

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

// THE argument checks of every entry, all answered -1 before a device is looked for: the options and the extras are plausible (a
// struct size; a weight_stride of 0 or m; for a kPlain entry neither weights nor covariance), the model has the derivative it is
// asked for (kRefusesAnalytic), no pointer is missing and t_stride is 0 or m. e: the extras as this build understands them;
// pass: what the entry hands on to the launch -- the caller's extras, or for a kPlain entry e cut down to its flag, or nullptr.
template <class Models, class Model, class T>
bool batched_entry_arguments(const void* S, size_t m, const T* x, const T* lower, const T* upper, const T* t, size_t t_stride, const T* data,
                             const void* results, const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras,
                             mir_lsq_batched_extras& e, const mir_lsq_batched_extras*& pass)
{
    if (!batched_options_plausible(options) || !mir_optim_amd::detail::batched_extras(extras, m, e)) return false;
    pass = extras;
    if (Models::kPlain) {
        if (e.weights || e.covariance) return false;
        const uint32_t flag = e.flags & MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM;
        e = mir_lsq_batched_extras{};
        e.struct_size = sizeof e; e.flags = flag;
        pass = flag ? &e : nullptr;
    }
    if (Models::kRefusesAnalytic && !batched_has_grad<Model>::value && (batched_options(options).variant & MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN))
        return false;
    return S && x && lower && upper && t && data && results && (t_stride == 0 || t_stride == m);
}

// the device-pointer fit entries (mir_lsq_batched_kernel_s / _d, _ex_s / _ex_d, mir_lsq_batched16_kernel_d / _ex_d)
template <class Models, class T = typename Models::value_type>
int batched_kernel_entry(const typename Abi<T>::Settings* S, size_t count, size_t m, int model, T* x, const T* lower, const T* upper,
                         const T* t, size_t t_stride, const T* data, typename Abi<T>::Result* results,
                         const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras = nullptr)
{
    return Models::with_model(model, [&](auto mdl) {
        using Model = decltype(mdl);
        mir_lsq_batched_extras e;
        const mir_lsq_batched_extras* pass;
        if (!batched_entry_arguments<Models, Model>(S, m, x, lower, upper, t, t_stride, data, results, options, extras, e, pass)) return -1;
        if (count != 0 && !device_available()) return -2;
        const mir_lsq_batched_options o = batched_options(options);
        return mir_optim_amd::detail::launch_fit_with<Model, typename Models::template Kernels<Model>>(S, count, m, x, lower, upper, t, t_stride,
                                                                                                       data, results, &o, pass);
    });
}

// the covariance kernel on its own (mir_lsq_batched_covariance_s / _d, mir_lsq_batched16_covariance_d)
template <class Models, class T = typename Models::value_type>
int batched_covariance_entry(const typename Abi<T>::Settings* S, size_t count, size_t m, int model, const T* x, const T* lower,
                             const T* upper, const T* t, size_t t_stride, const T* data, const typename Abi<T>::Result* results,
                             const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return Models::with_model(model, [&](auto mdl) {
        using Model = decltype(mdl);
        mir_lsq_batched_extras e;
        const mir_lsq_batched_extras* pass;
        if (!batched_entry_arguments<Models, Model>(S, m, x, lower, upper, t, t_stride, data, results, options, extras, e, pass) || !e.covariance)
            return -1;
        if (count != 0 && !device_available()) return -2;
        const mir_lsq_batched_options o = batched_options(options);
        return mir_optim_amd::detail::launch_covariance_with<Model, typename Models::template Kernels<Model>>(S, count, m, x, lower, upper, t,
                                                                                                              t_stride, data, results, &o, pass);
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

// THE host-pointer entry of one model, after the argument checks of batched_entry_arguments: one allocation, the uploads, the
// fit with the kernels of `Kernels`, the copies back. extras: HOST pointers, or nullptr.
// Where the layout of the model leaves problems for the general solver (n <= 8: status -100 for a step that reaches a finite
// bound) those are completed here, and the covariance is a launch of its own at every problem's FINAL x behind that; where it
// does not (9 <= n <= 16) the covariance rides on the fit's launch and that stage is not compiled in.
template <class Model, class Kernels, class T = batched_value_t<Model>>
int batched_host_model_entry(const typename Abi<T>::Settings* S, size_t count, size_t m, T* x, const T* lower, const T* upper,
                             const T* t, size_t t_stride, const T* data, typename Abi<T>::Result* results,
                             const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    using Result = typename Abi<T>::Result;
    using Layout = mir_optim_amd::detail::BatchedLayout<Model>;
    constexpr size_t n = Model::n;
    mir_lsq_batched_extras e;                  // HOST pointers here
    (void)mir_optim_amd::detail::batched_extras(extras, m, e);
    const T* weights = static_cast<const T*>(e.weights);
    T* cov = static_cast<T*>(e.covariance);
    const size_t wn = weights ? (e.weight_stride ? count : 1) * m : 0;
    for (size_t i = 0; i < wn; ++i)
        if (!(-Lim<T>::inf() < weights[i] && weights[i] < Lim<T>::inf())) return -1;      // non-finite weights: the caller's error
    for (size_t i = 0; i < count; ++i) {       // defaults of LeastSquaresResult!T, LS:132-142
        results[i].status = mir_ls_numericError; results[i].iterations = results[i].fCalls = results[i].gCalls = 0;
        results[i].residual = Lim<T>::inf(); results[i].lambda = 0;
    }
    if (count == 0) return 0;
    const int bad = bad_settings(S);           // common to all problems (the code is reported per problem)
    if (!device_available()) return -2;
    if (m == 0 || Layout::fit_lds_bytes(m) > mir_optim_amd::kBatchedLdsLimit) {
        std::fprintf(stderr, "[mir_optim_amd] batched %s entry, n = %zu: m = %zu does not fit one wave's LDS slice\n",
                     std::is_same<T, double>::value ? "f64" : "f32", n, m);
        return -3;
    }
    if (bad) {
        for (size_t i = 0; i < count; ++i) results[i].status = bad;
        for (size_t i = 0; cov && i < count * n * n; ++i) cov[i] = Lim<T>::inf() - Lim<T>::inf();   // negative status: NaN
        return 0;
    }
    mir_lsq_batched_options o = batched_options(options);
    o.stream = nullptr;
    // one allocation: the arrays, the records, the model's per-row basis table (values of T), the weights and the covariance
    const size_t basis_b = mir_optim_amd::batched_basis_floats<Model>(count, m, t_stride) * sizeof(T);
    const size_t tb = (t_stride ? count : 1) * m * sizeof(T), db = count * m * sizeof(T), xb = count * n * sizeof(T);
    const size_t wb = wn * sizeof(T), cb = cov ? count * n * n * sizeof(T) : 0;
    // MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM: lower / upper hold count x n values, row i the box of problem i
    const size_t bstep = (e.flags & MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM) ? n : 0, bb = (bstep ? count : 1) * n * sizeof(T);
    char* base = nullptr;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o_ = off; off = align_up(off + bytes, 256); return o_; };
    const size_t ot = take(tb), od = take(db), ox = take(xb), ol = take(bb), ou = take(bb),
                 orr = take(count * sizeof(Result)), obasis = take(basis_b), ow = take(wb), oc = take(cb);
    if (hipMalloc((void**)&base, off) != hipSuccess) return -4;
    o.basis = basis_b ? (float*)(base + obasis) : nullptr;      // the C member is float*; it holds doubles for a double model
    o.basis_bytes = basis_b;
    const T* dt = (const T*)(base + ot); const T* ddata = (const T*)(base + od); T* dx = (T*)(base + ox);
    const T* dlower = (const T*)(base + ol); const T* dupper = (const T*)(base + ou); const T* dw = wb ? (const T*)(base + ow) : nullptr;
    Result* dres = (Result*)(base + orr);      // the kernel writes the C records in place (the layout's checks assert it)
    // the device twin of the extras; its covariance rides on the fit's launch unless the general solver comes in between
    mir_lsq_batched_extras de{};
    de.struct_size = sizeof de; de.flags = e.flags; de.weights = dw; de.weight_stride = e.weight_stride;
    de.covariance = cb && !Layout::needs_general ? base + oc : nullptr;
    std::vector<T> x0;                         // starts, for the problems the general solver completes
    if (Layout::needs_general) x0.assign(x, x + count * n);
    bool good = hipMemcpy(base + ot, t, tb, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + od, data, db, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ox, x, xb, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ol, lower, bb, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy(base + ou, upper, bb, hipMemcpyHostToDevice) == hipSuccess
        && (!wb || hipMemcpy(base + ow, weights, wb, hipMemcpyHostToDevice) == hipSuccess)
        && mir_optim_amd::detail::launch_fit_with<Model, Kernels>(S, count, m, dx, dlower, dupper, dt, t_stride, ddata, dres, &o,
                                                                  extras ? &de : nullptr) == 0
        && hipDeviceSynchronize() == hipSuccess
        && hipMemcpy(results, dres, count * sizeof(Result), hipMemcpyDeviceToHost) == hipSuccess
        && hipMemcpy(x, dx, xb, hipMemcpyDeviceToHost) == hipSuccess;
    if constexpr (Layout::needs_general) {
        for (size_t i = 0; good && i < count; ++i) {
            if (results[i].status != kBatchedNeedsGeneral) continue;
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
        if (good && cov) {
            // the covariance at every problem's FINAL x: the records and x of the completed problems go back to the device first
            de.covariance = base + oc;
            good = hipMemcpy(dres, results, count * sizeof(Result), hipMemcpyHostToDevice) == hipSuccess
                && hipMemcpy(dx, x, xb, hipMemcpyHostToDevice) == hipSuccess
                && mir_optim_amd::detail::launch_covariance_with<Model, Kernels>(S, count, m, dx, dlower, dupper, dt, t_stride, ddata, dres, &o,
                                                                                 &de) == 0
                && hipDeviceSynchronize() == hipSuccess;
        }
    }
    good = good && (!cb || hipMemcpy(cov, base + oc, cb, hipMemcpyDeviceToHost) == hipSuccess);
    (void)hipFree(base);
    return good ? 0 : -5;
}

// the host-pointer entries (mir_optimize_least_squares_batched_s / _d, _ex_s / _ex_d, mir_optimize_least_squares_batched16_d / _ex_d)
template <class Models, class T = typename Models::value_type>
int batched_host_entry(const typename Abi<T>::Settings* S, size_t count, size_t m, int model, T* x, const T* lower, const T* upper,
                       const T* t, size_t t_stride, const T* data, typename Abi<T>::Result* results,
                       const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras = nullptr)
{
    return Models::with_model(model, [&](auto mdl) {
        using Model = decltype(mdl);
        mir_lsq_batched_extras e;
        const mir_lsq_batched_extras* pass;
        if (!batched_entry_arguments<Models, Model>(S, m, x, lower, upper, t, t_stride, data, results, options, extras, e, pass)) return -1;
        return batched_host_model_entry<Model, typename Models::template Kernels<Model>>(S, count, m, x, lower, upper, t, t_stride, data, results,
                                                                                         options, pass);
    });
}

}  // namespace mirlsq
