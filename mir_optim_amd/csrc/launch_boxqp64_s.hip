// launch_boxqp64_s.hip -- batched box-constrained QP solves of order 17 .. 64 in float (boxqp_wave.h: the matrices in LDS, the
// order a run-time argument): the two instances k_boxqp_wave<32, float> and k_boxqp_wave<64, float> and their extern "C" entries
// (boxqp_wave_launch.h). A translation unit of its own, as launch_boxqp16_s.hip is: no other unit recompiles or grows with it.
#include "boxqp_wave_launch.h"

using namespace mirlsq;

extern "C" {

int mir_lsq_batched_box_qp64_waves_s(const mir_box_qp_settings_s* settings, size_t count, size_t n, const float* P, const float* q,
                                     const float* l, const float* u, size_t bound_stride, float* x, int* status, int* iterations,
                                     unsigned flags, void* stream, unsigned max_waves)
{
    return batched_box_qp_wave_entry<float>(settings, count, n, P, q, l, u, bound_stride, x, status, iterations, flags, stream, max_waves);
}

int mir_lsq_batched_box_qp64_s(const mir_box_qp_settings_s* settings, size_t count, size_t n, const float* P, const float* q,
                               const float* l, const float* u, size_t bound_stride, float* x, int* status, int* iterations,
                               unsigned flags, void* stream)
{
    return batched_box_qp_wave_entry<float>(settings, count, n, P, q, l, u, bound_stride, x, status, iterations, flags, stream, 0);
}

}  // extern "C"
