// batched16_d.hip -- the batched one-wavefront-per-problem fit for models with 9 to 16 parameters (double; batched16_kernel.h,
// launch_batched16<Model> of include/mir_optim_amd_batched.hpp): the k_lm_batched16 instances of the two built-in models
// (MIR_LSQ_MODEL16_*), their extern "C" entries and the unit entry of the J^T J stage. A unit of its own, so that batched_d.hip
// compiles the device code it always compiled and the build stays parallel. The weighted instances, the covariance kernel and
// the entries that take weights and covariance are in batched16_ex_d.hip; the host layer of both is batched_host.h.
#include "batched_host.h"

using namespace mirlsq;

namespace {

// the kernels of this unit: the unweighted fit and nothing else
template <class Model> struct Batched16PlainKernels {
    static bool fit(const BatchedArgs<double>& a, bool weighted, size_t lds, hipStream_t stream)
    {
        return !weighted && mir_optim_amd::detail::launch_kernel(k_lm_batched16<Model>, dim3((unsigned)a.count), dim3(64), lds, stream, a);
    }
    static bool covariance(const BatchedCovArgs<double>&, size_t, hipStream_t) { return false; }
};

// these two entries take neither weights nor covariance (-1, as before the _ex entries of batched16_ex_d.hip existed); the
// per-problem-bounds bit of an extras passes: it needs no other kernel instance
using Models = BuiltinModels16<Batched16PlainKernels, true>;

}  // namespace

extern "C" {

int mir_lsq_batched16_kernel_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model, double* x,
                               const double* lower, const double* upper, const double* t, size_t t_stride, const double* data,
                               mir_least_squares_result_d* results, const mir_lsq_batched_options* options,
                               const mir_lsq_batched_extras* extras)
{
    return batched_kernel_entry<Models>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options, extras);
}

int mir_optimize_least_squares_batched16_d(const mir_least_squares_settings_d* S, size_t count, size_t m, int model, double* x,
                                           const double* lower, const double* upper, const double* t, size_t t_stride,
                                           const double* data, mir_least_squares_result_d* results,
                                           const mir_lsq_batched_options* options, const mir_lsq_batched_extras* extras)
{
    return batched_host_entry<Models>(S, count, m, model, x, lower, upper, t, t_stride, data, results, options, extras);
}

int mir_lsq_batched16_jtj_d(size_t count, size_t m, size_t n, const double* J, const double* y, double* JJ, double* Jy, void* stream)
{
    if (!J || !y || !JJ || !Jy || n < 1 || n > (size_t)kW16) return -1;
    if (count == 0) return 0;
    const size_t lds = ((size_t)(kW16 + 1) * m + kBatched16TileDoubles) * sizeof(double);
    if (m == 0 || lds > mir_optim_amd::kBatchedLdsLimit) return -3;
    if (!device_available()) return -2;
    if (!mir_optim_amd::detail::launch_kernel(k_batched16_jtj<>, dim3((unsigned)count), dim3(64), lds, static_cast<hipStream_t>(stream), (int)count,
                                              (int)m, (int)n, J, y, JJ, Jy))
        return -5;
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // extern "C"

// (after the entries: the kernels are then instantiated in the order in which this unit always emitted them)
bool mirlsq::batched16_plain_enqueue(int model, const BatchedArgs<double>& a, size_t lds, hipStream_t stream)
{
    return with_builtin_model16(model, [&](auto mdl) { return (int)Batched16PlainKernels<decltype(mdl)>::fit(a, false, lds, stream); }) == 1;
}
