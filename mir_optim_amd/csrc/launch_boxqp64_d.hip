// launch_boxqp64_d.hip -- batched box-constrained QP solves of order 17 .. 64 in double (boxqp_wave.h: the matrices in LDS,
// the order a run-time argument): the two instances k_boxqp_wave<32, double> and k_boxqp_wave<64, double> and their extern "C"
// entries (boxqp_wave_launch.h). A translation unit of its own, as launch_boxqp16_d.hip is.
#include "boxqp_wave_launch.h"

using namespace mirlsq;

extern "C" {

int mir_lsq_batched_box_qp64_waves_d(const mir_box_qp_settings_d* settings, size_t count, size_t n, const double* P, const double* q,
                                     const double* l, const double* u, size_t bound_stride, double* x, int* status, int* iterations,
                                     unsigned flags, void* stream, unsigned max_waves)
{
    return batched_box_qp_wave_entry<double>(settings, count, n, P, q, l, u, bound_stride, x, status, iterations, flags, stream, max_waves);
}

int mir_lsq_batched_box_qp64_d(const mir_box_qp_settings_d* settings, size_t count, size_t n, const double* P, const double* q,
                               const double* l, const double* u, size_t bound_stride, double* x, int* status, int* iterations,
                               unsigned flags, void* stream)
{
    return batched_box_qp_wave_entry<double>(settings, count, n, P, q, l, u, bound_stride, x, status, iterations, flags, stream, 0);
}

}  // extern "C"
