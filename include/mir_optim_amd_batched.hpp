// mir_optim_amd_batched.hpp -- the batched one-wavefront-per-problem LM fit as a DEVICE HEADER, for residual models of the
// caller's own (HIP C++, gfx950; compile with hipcc -I<repo>/include; the kernel sources under <repo>/mir_optim_amd/csrc travel with it).
//
// The reference takes an arbitrary residual function f (/root/reference/source/mir/optim/least_squares.d:73-80, C tier
// :705-724). The batched kernel (mir_optim_amd/csrc/batched_kernel.h) runs the whole loop of
// optimizeLeastSquaresImplGeneric!T (least_squares.d:877-1176) inside ONE kernel launch with the residual inlined, so a
// function pointer across the FFI is not an option there: the model is a compile-time type instead, and this header is the
// way to hand one in. The three models behind mir_optimize_least_squares_batched_s / mir_lsq_batched_kernel_s
// (MIR_LSQ_MODEL_*) are instances of the same template -- nothing about them is special.
//
// A model:
//     struct MyModel {
//         static constexpr int n  = 4;   // parameters, 1 <= n <= 8
//         static constexpr int nb = 0;   // per-row basis values that do not depend on the parameters (0 = none)
//         __device__ static void  basis(float t, float* b) {}                               // fills b[0 .. nb)
//         __device__ static float eval(float t, const float* b, const float* x)             // model value at t; x[n..8) = 0
//         { return x[0] * __expf(-t * x[1]) * __cosf(x[2] * t) + x[3]; }
//     };
// Optional, the reference's g callback: `__device__ static void grad(float t, const float* b, const float* x, float* g)` -- g[j] =
// d eval / d x_j, j < n -- used instead of finite differences when options->variant has MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN.
// Optional, the precision: `using value_type = double;` makes the whole fit double (LeastSquaresSettings!double, the reference's
// main instantiation) -- basis, eval and grad then take and return double, and launch_batched takes the _d settings and result
// records and double arrays, as mir_lsq_batched_kernel_d does. Without the member the model is float, as before.
// The residual of row i is eval(t_i, basis_i, x) - data_i. eval must be pure (as the reference's callbacks are declared)
// and free of lane-dependent control flow. A problem needs (n + 2) m values of LDS ((n + 2) m sizeof(T) <= 160 KB - 512: a
// double model at n = 8 reaches m = 2041).
// Reproducibility: the kernel's own arithmetic is a fixed sequence of IEEE operations (contraction off, every fused multiply-add
// written out: batched_kernel.h), so a fit is reproducible bit for bit on a host (oracle/lm_batched_fused.c does it for the
// built-in cfg 5 model) -- PROVIDED eval is written the same way: `#pragma clang fp contract(off)` as its first statement, explicit
// __builtin_fmaf, and no library transcendental whose bits differ between implementations (mirlsq::det_expf is one that does not).
// An eval written as in the example above is still deterministic on the device; only a host twin would differ in the last bit.
//
//     mir_optim_amd::launch_batched<MyModel>(&settings, count, m, x, lower, upper, t, t_stride, data, results, &options);
// has the contract of mir_lsq_batched_kernel_s / _d (include/mir_optim_amd.h): every pointer a DEVICE pointer, enqueued on
// options->stream, results in place, status -100 (MIR_LSQ_BATCHED_NEEDS_GENERAL) for a problem whose step reaches a finite
// bound. A caller with bounds that bind uses
//     mir_optim_amd::launch_batched_bounded<MyModel>(...the same arguments...);
// instead: it runs the bounded instance of the model's kernel, which solves the reference's box QP (BOXCQP, boxcqp.d:122-379)
// for such a step inside the kernel, so every problem is finished by the one launch and none returns -100. The two are separate
// templates so that a build which only calls launch_batched compiles the kernels it always compiled.
// tests/user_model/ holds complete examples that are compiled and compared with the oracle (user_model_bounded.hip: bounds).
//
// Weights and covariance (mir_lsq_batched_extras, the trailing argument of launch_batched; include/mir_optim_amd.h says the same
// of the C entries). With extras->weights the residual of row i is  w_i (eval(t_i, basis_i, x) - data_i)  -- w_i = 1 / sigma_i
// for data with per-point uncertainties -- in the residual, at both points of every central difference and as w_i grad_j on the
// analytic path: the fit the reference makes of a weighted f. weight_stride 0: one vector of m weights for all problems; m:
// count x m. A weight of exactly 0 removes its row; problems of different lengths are padded to a common m with zero-weight
// rows (finite data there). The weighted kernel is an instance of its own (k_lm_batched<Model, true>): an unweighted launch
// runs the code it always ran. With extras->covariance the launch is followed, on the same stream, by
// launch_batched_covariance<Model>: per problem n x n values, cov = s^2 (J^T J)^-1 with J the weighted Jacobian at the final x
// (grad or central differences, as the fit's options say) and s^2 = residual / (rows with nonzero weight - n), or s^2 = 1 with
// MIR_LSQ_BATCHED_ABSOLUTE_SIGMA; +inf everywhere when J^T J is not positive definite or the degrees of freedom are <= 0, NaN
// everywhere for a problem with a negative status (-100 included: finish it, then call launch_batched_covariance -- or fit with
// launch_batched_bounded, which leaves no such problem).
// tests/user_model/user_model_weighted.hip is the example.
//
// Per-problem bounds and fixed parameters. With MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM in extras->flags (an extras with nothing else
// is valid) `lower` and `upper` hold count x n values, row k being problem k's box; without it n values serve every problem.
// Every launch_* of this file honours the bit: the kernels take `lower + prob * n` once at entry (k_lm_batched in instances of
// their own, k_lm_batched<Model, WEIGHTED, Bounds, true>, so that a shared-bounds launch runs the code it always ran; the other
// kernels through a run-time stride of 0 or n), so a launch whose rows are all equal gives the bits of the shared launch, and each problem is validated against its own row
// (boundsError, -32, for that problem alone). A parameter with l_j == u_j in its problem's box is FIXED: the fit keeps it at
// that value, and in the covariance its row and column are exactly 0, the other entries are the reduced problem's covariance
// and s^2 divides by rows - n_free; +inf then fills the free entries only. One that ends on a bound with l_j < u_j is not fixed.
// tests/user_model/user_model_problem_bounds.hip is the example.
//
// Models with 9 to 16 parameters (double only): launch_batched16<Model>, at the end of this file. The model contract is the one
// above with `using value_type = double;`, 9 <= n <= 16 and 16 entries in x (x[n..16) = 0); the kernel is a different one
// (mir_optim_amd/csrc/batched16_kernel.h: J^T J on the matrix unit, the n x n work in the 16-lane-row layout, bounds always
// handled in the kernel) and takes (16 + 2) m + 272 doubles of LDS: m <= 1119. tests/user_model/user_model_n16.hip is the example.
// Weights and covariance work as above through the trailing extras of launch_batched16 and launch_batched16_covariance<Model>
// (k_lm_batched16<Model, true>, k_batched16_covariance<Model>); tests/user_model/user_model_n16_weighted.hip is the example.
//
// The fitted curve and its confidence band: launch_batched_predict<Model>, at the end of this file, for a model of either width.
// With x (count x n) and the covariance (count x n x n) a fit left on the device, and q abscissae of the caller's choice (one
// grid for the batch or one per problem), it writes  value = eval(tq_i; x_k)  and, where wanted,  sigma = sqrt(g^T C_k g),
// g = d eval / d x at tq_i -- the 1-sigma band of the curve, what a curve-fit front end's eval_uncertainty computes -- with the
// model's own grad (MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN) or the central differences, clipped to the box, that built the
// covariance; a fixed parameter (l_j == u_j) contributes nothing and its row and column of the covariance are not read. The
// covariance's conventions pass through: +inf for a problem whose covariance is +inf, NaN for one whose fit failed; value is
// written for every problem. One kernel (mir_optim_amd/csrc/batched_predict.h: a wave per problem, a query per lane), one launch,
// no allocation, no synchronisation. tests/user_model/user_model_predict.hip is the example.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <type_traits>

#include "mir_optim_amd.h"
#include "../mir_optim_amd/csrc/batched_kernel.h"
#include "../mir_optim_amd/csrc/batched_bounded.h"
#include "../mir_optim_amd/csrc/batched16_kernel.h"
#include "../mir_optim_amd/csrc/batched_predict.h"

namespace mir_optim_amd {

// the value type of a model (float unless it declares `using value_type = double;`) and the C records that go with it
template <class Model> using batched_value_t = mirlsq::batched_value_t<Model>;
template <class Model>
using batched_settings_t = std::conditional_t<std::is_same<batched_value_t<Model>, double>::value, mir_least_squares_settings_d,
                                              mir_least_squares_settings_s>;
template <class Model>
using batched_result_t = std::conditional_t<std::is_same<batched_value_t<Model>, double>::value, mir_least_squares_result_d,
                                            mir_least_squares_result_s>;

// LDS bytes one problem of `Model` needs at m rows; launch_batched returns -3 when it exceeds kBatchedLdsLimit
constexpr size_t kBatchedLdsLimit = 160 * 1024 - 512;
template <class Model> constexpr size_t batched_lds_bytes(size_t m) { return (size_t)(Model::n + 2) * m * sizeof(batched_value_t<Model>); }
// values (of the model's type: floats, or doubles for a double model) of the per-row basis table a launch needs (0 for a model
// without a basis): mir_lsq_batched_options.basis, whose basis_bytes is this times sizeof(batched_value_t<Model>)
template <class Model> constexpr size_t batched_basis_floats(size_t count, size_t m, size_t t_stride)
{
    return (size_t)Model::nb * (t_stride ? count : 1) * m;
}

namespace detail {
// the extras as this build understands them (struct_size-versioned); false: implausible
inline bool batched_extras(const mir_lsq_batched_extras* extras, size_t m, mir_lsq_batched_extras& e)
{
    e = mir_lsq_batched_extras{};
    if (!extras) return true;
    if (extras->struct_size < 8 || extras->struct_size > 1024) return false;
    std::memcpy(&e, extras, extras->struct_size < sizeof e ? extras->struct_size : sizeof e);
    e.struct_size = sizeof e;
    return e.weight_stride == 0 || e.weight_stride == m;
}
// the stride of lower / upper in the kernels' arguments: n with MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM (count x n values), else 0
template <class Model> constexpr int bound_stride(const mir_lsq_batched_extras& e)
{
    return (e.flags & MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM) ? Model::n : 0;
}

// The per-row basis table of a launch: the caller's (options->basis) or one of this call's own.
// No table from the caller: hipMalloc, and a stream synchronisation before hipFree in release(). (Until round 4 this was
// hipMallocAsync / hipFreeAsync, and 2 of 300 calls with a 2 MB table returned wrong fits for a contiguous range of
// problems. Root cause, reproduced WITHOUT any library code by scripts/probes/malloc_async_probe.hip on this ROCm
// (HIP runtime 70226015): with the pool's default release threshold (0) a synchronisation hands the freed block back
// to the OS, the next hipMallocAsync maps memory at the same address again, and kernels then read wrong words from
// it -- 84 % of a table per iteration when ordinary hipMalloc / hipFree traffic runs beside it, still some without;
// with hipMemPoolAttrReleaseThreshold = UINT64_MAX (the pool keeps its memory): none, in any configuration
// (profiles/r05/malloc_async_probe_*.txt). The runtime's, not this library's; a caller who wants stream-ordered
// allocation around these launches raises that threshold first. The table here stays in ordinary memory:
// tests/test_gpu_batched.py::test_repeated_launches_with_a_large_basis_table_agree.)
template <class Model> struct BasisTable {
    using T = batched_value_t<Model>;
    T* table = nullptr;
    bool owned = false;
    // 0, or -1 (the caller's table is too small) / -4 (allocation)
    int acquire(const mir_lsq_batched_options* opt, const T* t, size_t count, size_t m, size_t t_stride, hipStream_t stream)
    {
        if constexpr (Model::nb > 0) {
            const size_t rows = (size_t)(t_stride ? count : 1) * m, bytes = rows * Model::nb * sizeof(T);
            if (opt && opt->basis) {
                if (opt->basis_bytes < bytes) return -1;
                table = reinterpret_cast<T*>(opt->basis);          // the caller's table (doubles for a double model): no allocation here
            } else {
                owned = true;
                if (hipMalloc((void**)&table, bytes) != hipSuccess) return -4;
            }
            const unsigned bb = (unsigned)std::min<size_t>((rows + 255) / 256, 4096);
            hipLaunchKernelGGL(mirlsq::k_batched_basis<Model>, dim3(bb), dim3(256), 0, stream, t, table, rows);
        }
        return 0;
    }
    hipError_t release(hipStream_t stream, hipError_t e)
    {
        if (owned) {
            const hipError_t f = hipStreamSynchronize(stream);     // the kernels read the table: wait before freeing it
            (void)hipFree(table);
            if (e == hipSuccess) e = f;
        }
        return e;
    }
};

// THE launch of a kernel with `lds` bytes of dynamic LDS: above the 48 KB a kernel may take by default its limit is raised first
// (at or below it no attribute call is made). false: the limit could not be raised and nothing was launched.
template <class Kernel, class... Args>
bool launch_kernel(Kernel kern, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args&... args)
{
    if (lds > 48 * 1024
        && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return false;
    hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
    return true;
}
}  // namespace detail

// ---- 9 <= n <= 16, double: k_lm_batched16 (mir_optim_amd/csrc/batched16_kernel.h) --------------------------------------------
// LDS bytes one problem needs at m rows: J with a row stride of 16, y, the trial residual, the 16 x 16 J^T J tile and J^T y.
// launch_batched16 returns -3 when it exceeds kBatchedLdsLimit: (16 + 2) 8 m + 2176 <= 160 KB - 512, m <= kBatched16MaxRows.
template <class Model> constexpr size_t batched16_lds_bytes(size_t m)
{
    return ((size_t)(mirlsq::kW16 + 2) * m + mirlsq::kBatched16TileDoubles) * sizeof(double);
}
constexpr size_t kBatched16MaxRows = (kBatchedLdsLimit - mirlsq::kBatched16TileDoubles * sizeof(double)) / ((mirlsq::kW16 + 2) * sizeof(double));
static_assert(kBatched16MaxRows == 1119, "the m limit the headers document");

// LDS bytes of the covariance kernel of these models (k_batched16_covariance: J, one m-vector, the tile): below the fit's.
constexpr size_t batched16_covariance_lds_bytes(size_t m)
{
    return ((size_t)(mirlsq::kW16 + 1) * m + mirlsq::kBatched16TileDoubles) * sizeof(double);
}

namespace detail {
// A launch takes its kernel instances from a policy class `Kernels`:
//     static bool fit(const BatchedArgs<T>&, bool weighted, size_t lds, hipStream_t);      false: the launch could not be made
//     static bool covariance(const BatchedCovArgs<T>&, size_t lds, hipStream_t);
// These two are every instance of a model; the library's translation units have policies of their own, which forward what they
// do not compile to the unit that does (mir_optim_amd/csrc/batched_host.h), so that each unit compiles the device code it
// always compiled.
// n <= 8: k_lm_batched, weighted or not, with the bounded step (Bounds = BatchedBoxQpStep) or without
template <class Model, class Bounds> struct BatchedKernels {
    using T = batched_value_t<Model>;
    static bool fit(const mirlsq::BatchedArgs<T>& a, bool weighted, size_t lds, hipStream_t stream)
    {
        // the host picks the instance: weighted or not, one box for the batch or a row per problem
        auto kern = a.b_stride ? (weighted ? mirlsq::k_lm_batched<Model, true, Bounds, true> : mirlsq::k_lm_batched<Model, false, Bounds, true>)
                               : (weighted ? mirlsq::k_lm_batched<Model, true, Bounds> : mirlsq::k_lm_batched<Model, false, Bounds>);
        return launch_kernel(kern, dim3((unsigned)a.count), dim3(64), lds, stream, a);
    }
    static bool covariance(const mirlsq::BatchedCovArgs<T>& c, size_t lds, hipStream_t stream)
    {
        return launch_kernel(mirlsq::k_batched_covariance<Model>, dim3((unsigned)c.count), dim3(64), lds, stream, c);
    }
};
// 9 <= n <= 16: k_lm_batched16 (bounds always handled in the kernel)
template <class Model> struct Batched16Kernels {
    static bool fit(const mirlsq::BatchedArgs<double>& a, bool weighted, size_t lds, hipStream_t stream)
    {
        auto kern = weighted ? mirlsq::k_lm_batched16<Model, true> : mirlsq::k_lm_batched16<Model, false>;   // the host picks the instance
        return launch_kernel(kern, dim3((unsigned)a.count), dim3(64), lds, stream, a);
    }
    static bool covariance(const mirlsq::BatchedCovArgs<double>& c, size_t lds, hipStream_t stream)
    {
        return launch_kernel(mirlsq::k_batched16_covariance<Model>, dim3((unsigned)c.count), dim3(64), lds, stream, c);
    }
};

// The kernel family ("layout") a model belongs to, by its n: what differs between the two in the host code of a launch.
template <class Model, bool kWide = (Model::n > mirlsq::kBatchedNMax)> struct BatchedLayout;
template <class Model> struct BatchedLayout<Model, false> {        // n <= 8: one matrix row per lane of a group of eight
    using Kernels = BatchedKernels<Model, mirlsq::BatchedNoBoundedStep>;        // the default set: launch_batched
    // a problem whose step reaches a finite bound may come back with status -100 (unless the bounded instances run), and
    // k_lm_batched reads mir_lsq_batched_options.timing
    static constexpr bool needs_general = true, has_timing = true;
    static constexpr void checks()
    {
        using namespace mirlsq;
        using T = batched_value_t<Model>;
        static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value, "Model::value_type: float or double");
        static_assert(Model::n >= 1 && Model::n <= kBatchedNMax, "1 <= n <= 8: one matrix row per lane of a group of eight");
        static_assert(Model::nb >= 0, "nb: number of per-row basis values");
        static_assert(sizeof(BatchedResult<T>) == sizeof(batched_result_t<Model>), "the kernel writes the C result records in place");
        static_assert(offsetof(BatchedResult<T>, residual) == offsetof(batched_result_t<Model>, residual)
                      && offsetof(BatchedResult<T>, lambda) == offsetof(batched_result_t<Model>, lambda), "same layout as the C record");
    }
    static constexpr size_t fit_lds_bytes(size_t m) { return batched_lds_bytes<Model>(m); }
    static constexpr size_t covariance_lds_bytes(size_t) { return 0; }
    static constexpr bool covariance_fits(size_t m) { return m != 0; }
};
template <class Model> struct BatchedLayout<Model, true> {         // 9 <= n <= 16, double: the 16-lane-row layout
    using Kernels = Batched16Kernels<Model>;
    static constexpr bool needs_general = false, has_timing = false;
    static constexpr void checks()
    {
        using namespace mirlsq;
        static_assert(std::is_same<batched_value_t<Model>, double>::value, "launch_batched16: Model::value_type must be double");
        static_assert(Model::n >= kBatched16NMin && Model::n <= kBatched16NMax, "9 <= n <= 16 (launch_batched takes n <= 8)");
        static_assert(Model::nb >= 0, "nb: number of per-row basis values");
        static_assert(sizeof(BatchedResult<double>) == sizeof(mir_least_squares_result_d)
                      && offsetof(BatchedResult<double>, residual) == offsetof(mir_least_squares_result_d, residual)
                      && offsetof(BatchedResult<double>, lambda) == offsetof(mir_least_squares_result_d, lambda),
                      "the kernel writes the C result records in place");
    }
    static constexpr size_t fit_lds_bytes(size_t m) { return batched16_lds_bytes<Model>(m); }
    static constexpr size_t covariance_lds_bytes(size_t m) { return batched16_covariance_lds_bytes(m); }
    static constexpr bool covariance_fits(size_t m) { return m != 0 && fit_lds_bytes(m) <= kBatchedLdsLimit; }   // the fit's limit: the records come from one
};

// the arguments of the fit kernel; timing: mir_lsq_batched_options.timing where the kernel reads it (k_lm_batched), else nullptr
template <class Model, class T = batched_value_t<Model>>
mirlsq::BatchedArgs<T> fit_args(const batched_settings_t<Model>* S, size_t count, size_t m, T* x, const T* lower, const T* upper, const T* t,
                                size_t t_stride, const T* data, batched_result_t<Model>* results, const T* table, uint32_t variant,
                                uint64_t* timing, const mir_lsq_batched_extras& e)
{
    mirlsq::BatchedArgs<T> a{};
    a.set = mirlsq::lm_settings_dev(S);
    a.maxIterations = S->maxIterations; a.maxAge = S->maxAge;
    a.count = (int)count; a.m = (int)m; a.t_stride = (int)t_stride;
    a.variant = variant;
    a.timing = timing;
    a.t = t; a.data = data; a.x = x; a.lower = lower; a.upper = upper;
    a.results = reinterpret_cast<mirlsq::BatchedResult<T>*>(results);
    a.weights = static_cast<const T*>(e.weights); a.w_stride = (int)e.weight_stride;
    a.b_stride = bound_stride<Model>(e);
    a.basis = table;
    return a;
}
// the arguments of the covariance kernel
template <class Model, class T = batched_value_t<Model>>
mirlsq::BatchedCovArgs<T> cov_args(const batched_settings_t<Model>* S, size_t count, size_t m, const T* x, const T* lower, const T* upper,
                                   const T* t, size_t t_stride, const T* data, const batched_result_t<Model>* results, const T* table,
                                   uint32_t variant, const mir_lsq_batched_extras& e)
{
    mirlsq::BatchedCovArgs<T> c{};
    c.jacobianEpsilon = S->jacobianEpsilon;
    c.count = (int)count; c.m = (int)m; c.t = t; c.t_stride = (int)t_stride; c.data = data; c.x = x; c.lower = lower; c.upper = upper;
    c.results = reinterpret_cast<const mirlsq::BatchedResult<T>*>(results);
    c.basis = table;
    c.weights = static_cast<const T*>(e.weights); c.w_stride = (int)e.weight_stride;
    c.variant = variant; c.flags = e.flags;
    c.cov = static_cast<T*>(e.covariance);
    c.b_stride = bound_stride<Model>(e);
    return c;
}

// THE launch of a fit, for the kernels of `Kernels`: the checks, the stream, the basis table, the fit, with extras->covariance the
// covariance behind it, the release and the return code. The public launch_* below are this with a layout and a kernel set.
template <class Model, class Kernels, class Layout = BatchedLayout<Model>, class T = batched_value_t<Model>>
int launch_fit_with(const batched_settings_t<Model>* S, size_t count, size_t m, T* x, const T* lower, const T* upper, const T* t,
                    size_t t_stride, const T* data, batched_result_t<Model>* results, const mir_lsq_batched_options* opt,
                    const mir_lsq_batched_extras* extras)
{
    Layout::checks();
    if (opt && (opt->variant & MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN) && !mirlsq::batched_has_grad<Model>::value) return -1;
    mir_lsq_batched_extras e;
    if (!batched_extras(extras, m, e)) return -1;
    if (!S || !x || !lower || !upper || !t || !data || !results || (t_stride != 0 && t_stride != m)) return -1;
    if (count == 0) return 0;
    const size_t lds = Layout::fit_lds_bytes(m);
    if (m == 0 || lds > kBatchedLdsLimit) return -3;
    hipStream_t stream = opt ? static_cast<hipStream_t>(opt->stream) : nullptr;
    const uint32_t variant = opt ? opt->variant : 0;
    BasisTable<Model> basis;
    if (const int rc = basis.acquire(opt, t, count, m, t_stride, stream)) return rc;
    bool launched = Kernels::fit(fit_args<Model>(S, count, m, x, lower, upper, t, t_stride, data, results, basis.table, variant,
                                                 Layout::has_timing && opt ? opt->timing : nullptr, e),
                                 e.weights != nullptr, lds, stream);
    if (launched && e.covariance)
        launched = Kernels::covariance(cov_args<Model>(S, count, m, x, lower, upper, t, t_stride, data, results, basis.table, variant, e),
                                       Layout::covariance_lds_bytes(m), stream);
    const hipError_t err = basis.release(stream, launched ? hipGetLastError() : hipErrorLaunchFailure);
    return err == hipSuccess ? 0 : -5;
}

// THE launch of the covariance kernel on its own, at the x and the records a fit left
template <class Model, class Kernels, class Layout = BatchedLayout<Model>, class T = batched_value_t<Model>>
int launch_covariance_with(const batched_settings_t<Model>* S, size_t count, size_t m, const T* x, const T* lower, const T* upper,
                           const T* t, size_t t_stride, const T* data, const batched_result_t<Model>* results,
                           const mir_lsq_batched_options* opt, const mir_lsq_batched_extras* extras)
{
    Layout::checks();
    if (opt && (opt->variant & MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN) && !mirlsq::batched_has_grad<Model>::value) return -1;
    mir_lsq_batched_extras e;
    if (!batched_extras(extras, m, e) || !e.covariance) return -1;          // (no extras: no covariance)
    if (!S || !x || !lower || !upper || !t || !data || !results || (t_stride != 0 && t_stride != m)) return -1;
    if (count == 0) return 0;
    if (!Layout::covariance_fits(m)) return -3;
    hipStream_t stream = opt ? static_cast<hipStream_t>(opt->stream) : nullptr;
    BasisTable<Model> basis;
    if (const int rc = basis.acquire(opt, t, count, m, t_stride, stream)) return rc;
    const bool launched = Kernels::covariance(cov_args<Model>(S, count, m, x, lower, upper, t, t_stride, data, results, basis.table,
                                                              opt ? opt->variant : 0, e),
                                              Layout::covariance_lds_bytes(m), stream);
    const hipError_t err = basis.release(stream, launched ? hipGetLastError() : hipErrorLaunchFailure);
    return err == hipSuccess ? 0 : -5;
}
}  // namespace detail

// Returns 0, or: -1 bad arguments, -3 a problem does not fit its workgroup's LDS, -4 allocation of the basis table failed,
// -5 the launch failed. Does not synchronise (except in the documented hipMalloc fallback of the basis table).
// A float model takes the _s records and float arrays, a double model the _d records and double arrays.
// extras (optional): per-row weights and / or the covariance of the fitted parameters, DEVICE pointers (see the top of this file).
// It instantiates the default kernels of the model only: with MIR_LSQ_BATCHED_DEVICE_BOUNDS in options->variant it returns -1
// (call launch_batched_bounded).
template <class Model>
int launch_batched(const batched_settings_t<Model>* S, size_t count, size_t m, batched_value_t<Model>* x,
                   const batched_value_t<Model>* lower, const batched_value_t<Model>* upper, const batched_value_t<Model>* t,
                   size_t t_stride, const batched_value_t<Model>* data, batched_result_t<Model>* results,
                   const mir_lsq_batched_options* opt = nullptr, const mir_lsq_batched_extras* extras = nullptr)
{
    if (opt && (opt->variant & MIR_LSQ_BATCHED_DEVICE_BOUNDS)) return -1;
    using Layout = detail::BatchedLayout<Model, false>;
    return detail::launch_fit_with<Model, typename Layout::Kernels, Layout>(S, count, m, x, lower, upper, t, t_stride, data, results, opt, extras);
}

// launch_batched with the BOUNDED instance of the model's kernel (csrc/batched_bounded.h): a damped step that leaves the box is
// replaced, inside the kernel, by the solution of the reference's box QP (least_squares.d:1074-1085, boxcqp.d:122-379 with
// settings->qpSettings), so no problem returns -100; a QP that does not end as solved ends its fit with numericError (-26), as
// in the reference. Same arguments and return codes; MIR_LSQ_BATCHED_DEVICE_BOUNDS in options->variant is accepted and not
// needed. A problem whose steps stay inside the box takes the steps, bit for bit, of launch_batched.
template <class Model>
int launch_batched_bounded(const batched_settings_t<Model>* S, size_t count, size_t m, batched_value_t<Model>* x,
                           const batched_value_t<Model>* lower, const batched_value_t<Model>* upper, const batched_value_t<Model>* t,
                           size_t t_stride, const batched_value_t<Model>* data, batched_result_t<Model>* results,
                           const mir_lsq_batched_options* opt = nullptr, const mir_lsq_batched_extras* extras = nullptr)
{
    return detail::launch_fit_with<Model, detail::BatchedKernels<Model, mirlsq::BatchedBoxQpStep>, detail::BatchedLayout<Model, false>>(
        S, count, m, x, lower, upper, t, t_stride, data, results, opt, extras);
}

// The covariance of the fitted parameters on its own: x (count x n) and results (the fit's records: status and residual are
// read) as a launch_batched left them -- or as the caller completed them for the -100 problems -- give extras->covariance
// (required; count x n x n values). Device pointers, enqueued on options->stream; the same return codes as launch_batched
// (-3: m = 0 only).
template <class Model>
int launch_batched_covariance(const batched_settings_t<Model>* S, size_t count, size_t m, const batched_value_t<Model>* x,
                              const batched_value_t<Model>* lower, const batched_value_t<Model>* upper,
                              const batched_value_t<Model>* t, size_t t_stride, const batched_value_t<Model>* data,
                              const batched_result_t<Model>* results, const mir_lsq_batched_options* opt,
                              const mir_lsq_batched_extras* extras)
{
    using Layout = detail::BatchedLayout<Model, false>;
    return detail::launch_covariance_with<Model, typename Layout::Kernels, Layout>(S, count, m, x, lower, upper, t, t_stride, data, results, opt,
                                                                                   extras);
}

// the residual vector of ONE problem, y_i = eval(t_i, basis_i, x) - data_i -- times w_i when `weights` (the problem's m values)
// is given -- as a kernel launch on device pointers: what a caller hands to the general solver as its device callback when a
// batched problem comes back with status -100 (float or double, as the model is: mir_optimize_least_squares_gpu_s / _d)
template <class Model>
void launch_model_residual(const batched_value_t<Model>* t, const batched_value_t<Model>* data, const batched_value_t<Model>* x,
                           batched_value_t<Model>* y, size_t m, hipStream_t stream, const batched_value_t<Model>* weights = nullptr)
{
    hipLaunchKernelGGL(mirlsq::k_batched_model_eval<Model>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, t, data, x, y, (int)m,
                       weights);
}

// launch_batched for a double model with 9 to 16 parameters. Same contract: every pointer a DEVICE pointer, enqueued on
// options->stream, results in place, no synchronisation except in the hipMalloc fallback of the basis table. Returns 0, or -1
// bad arguments (also MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN for a model without grad, and implausible extras), -3 m = 0 or above
// kBatched16MaxRows, -4 allocation of the basis table, -5 a launch failed. Finite bounds are handled inside the kernel (the
// reference's box QP, boxcqp.d:122-379): no problem returns -100; every solve is made for one damping value.
// MIR_LSQ_BATCHED_NO_LADDER and MIR_LSQ_BATCHED_DEVICE_BOUNDS are accepted and change nothing.
// extras (optional, DEVICE pointers), as for launch_batched: with extras->weights the weighted instance of the kernel runs
// (k_lm_batched16<Model, true>; an unweighted launch runs the code it always ran); with extras->covariance the fit is followed,
// on the same stream, by launch_batched16_covariance<Model>: count x n x n values, +inf / NaN in the degenerate cases named at
// the top of this file. tests/user_model/user_model_n16_weighted.hip is the example.
template <class Model>
int launch_batched16(const mir_least_squares_settings_d* S, size_t count, size_t m, double* x, const double* lower, const double* upper,
                     const double* t, size_t t_stride, const double* data, mir_least_squares_result_d* results,
                     const mir_lsq_batched_options* opt = nullptr, const mir_lsq_batched_extras* extras = nullptr)
{
    using Layout = detail::BatchedLayout<Model, true>;
    return detail::launch_fit_with<Model, typename Layout::Kernels, Layout>(S, count, m, x, lower, upper, t, t_stride, data, results, opt, extras);
}

// The covariance of the fitted parameters on its own, the counterpart of launch_batched_covariance: x (count x n) and results
// (status and residual are read) as a launch_batched16 left them give extras->covariance (required; count x n x n doubles).
// Device pointers, enqueued on options->stream; the return codes of launch_batched16.
template <class Model, class Kernels = detail::Batched16Kernels<Model>>
int launch_batched16_covariance(const mir_least_squares_settings_d* S, size_t count, size_t m, const double* x, const double* lower,
                                const double* upper, const double* t, size_t t_stride, const double* data,
                                const mir_least_squares_result_d* results, const mir_lsq_batched_options* opt,
                                const mir_lsq_batched_extras* extras)
{
    return detail::launch_covariance_with<Model, Kernels, detail::BatchedLayout<Model, true>>(S, count, m, x, lower, upper, t, t_stride, data,
                                                                                              results, opt, extras);
}

// ---- the fitted curve and its 1-sigma band on a grid of abscissae: k_batched_predict (mir_optim_amd/csrc/batched_predict.h) ----
namespace detail {
// THE argument checks of a prediction, all answered -1: the model has the derivative it is asked for; the extras are plausible and
// carry neither weights nor a covariance pointer (the covariance is an argument here; their flags pass); x, tq and value are
// there; lower and upper are both NULL or both given; sigma comes with a covariance; tq_stride is 0 or q; count, q < 2^31.
template <class Model, class T = batched_value_t<Model>>
bool predict_arguments(const void* S, size_t count, size_t q, const T* x, const T* lower, const T* upper, const T* tq, size_t tq_stride,
                       const T* covariance, const T* value, const T* sigma, const mir_lsq_batched_options* opt,
                       const mir_lsq_batched_extras* extras, mir_lsq_batched_extras& e)
{
    if (opt && (opt->variant & MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN) && !mirlsq::batched_has_grad<Model>::value) return false;
    if (!batched_extras(extras, 0, e) || e.weights || e.covariance) return false;
    if (!S || !x || !tq || !value || (lower == nullptr) != (upper == nullptr) || (sigma && !covariance)) return false;
    return (tq_stride == 0 || tq_stride == q) && count < ((size_t)1 << 31) && q < ((size_t)1 << 31);
}
}  // namespace detail

// value (count x q) = eval(tq_i; x_k) and, when `sigma` (count x q) is given, sigma = sqrt(max(0, g^T C_k g)) with C_k =
// covariance + k n^2 (count x n x n values, as the covariance entries write them; required with sigma) -- see the top of this
// file. Every pointer is a DEVICE pointer; the one launch is enqueued on options->stream; no allocation, no synchronisation.
// tq: q values for all problems (tq_stride 0) or count x q (tq_stride q). lower / upper: both NULL (unbounded, nothing fixed) or
// both given, n values, or count x n with MIR_LSQ_BATCHED_BOUNDS_PER_PROBLEM in extras->flags; they clip the difference points
// as in the fit, and l_j == u_j fixes parameter j. settings->jacobianEpsilon is the step of the differences;
// options->variant: MIR_LSQ_BATCHED_ANALYTIC_JACOBIAN. A model of any width: n <= 8 in float or double, 9 <= n <= 16 in double.
// Returns 0 (also for count == 0 or q == 0: nothing is launched), -1 bad arguments (detail::predict_arguments), -5 the launch failed.
template <class Model>
int launch_batched_predict(const batched_settings_t<Model>* S, size_t count, size_t q, const batched_value_t<Model>* x,
                           const batched_value_t<Model>* lower, const batched_value_t<Model>* upper,
                           const batched_value_t<Model>* tq, size_t tq_stride, const batched_value_t<Model>* covariance,
                           batched_value_t<Model>* value, batched_value_t<Model>* sigma, const mir_lsq_batched_options* opt = nullptr,
                           const mir_lsq_batched_extras* extras = nullptr)
{
    using T = batched_value_t<Model>;
    detail::BatchedLayout<Model>::checks();
    mir_lsq_batched_extras e;
    if (!detail::predict_arguments<Model>(S, count, q, x, lower, upper, tq, tq_stride, covariance, value, sigma, opt, extras, e)) return -1;
    if (count == 0 || q == 0) return 0;
    mirlsq::BatchedPredictArgs<T> a{};
    a.jacobianEpsilon = S->jacobianEpsilon;
    a.count = (int)count; a.q = (int)q;
    a.x = x; a.lower = lower; a.upper = upper; a.b_stride = lower ? detail::bound_stride<Model>(e) : 0;
    a.tq = tq; a.tq_stride = (int)tq_stride;
    a.variant = opt ? opt->variant : 0;
    a.cov = covariance; a.value = value; a.sigma = sigma;
    // a wave per problem and slice of the chunks of 64 queries: enough slices for ~8192 waves in flight, each keeping its C
    const size_t chunks = (q + 63) / 64, slices = std::min<size_t>(chunks, std::min<size_t>((8192 + count - 1) / count, 65535));
    hipLaunchKernelGGL(mirlsq::k_batched_predict<Model>, dim3((unsigned)count, (unsigned)slices), dim3(64), 0,
                       opt ? static_cast<hipStream_t>(opt->stream) : nullptr, a);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace mir_optim_amd
