// launch_boxqp16_s.hip -- batched box-constrained QP solves of order 9 .. 16 in float, four problems a wave (boxqp_rows16.h):
// the eight instances of k_boxqp_rows16 and of k_posvx_rows16 and their extern "C" entries (boxqp_launch.h). A translation
// unit of its own, as launch_boxqp.hip is: no other unit recompiles or grows with it.
#include "boxqp_launch.h"

using namespace mirlsq;

extern "C" {

int mir_lsq_batched_box_qp16_s(const mir_box_qp_settings_s* settings, size_t count, size_t n, const float* P, const float* q,
                               const float* l, const float* u, size_t bound_stride, float* x, int* status, int* iterations,
                               unsigned flags, void* stream)
{
    return batched_box_qp_entry<16, float>(settings, count, n, P, q, l, u, bound_stride, x, status, iterations, flags, stream);
}

int mir_lsq_batched_posvx16_s(size_t count, size_t n, const float* P, const float* rhs, float* x, int* info, void* stream)
{
    return batched_posvx16_entry<float>(count, n, P, rhs, x, info, stream);
}

}  // extern "C"
