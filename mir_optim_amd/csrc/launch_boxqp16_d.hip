// launch_boxqp16_d.hip -- batched box-constrained QP solves of order 9 .. 16 in double, four problems a wave (boxqp_rows16.h):
// the eight instances of k_boxqp_rows16 and of k_posvx_rows16 and their extern "C" entries (boxqp_launch.h). A translation
// unit of its own, as launch_boxqp.hip is: no other unit recompiles or grows with it.
#include "boxqp_launch.h"

using namespace mirlsq;

extern "C" {

int mir_lsq_batched_box_qp16_d(const mir_box_qp_settings_d* settings, size_t count, size_t n, const double* P, const double* q,
                               const double* l, const double* u, size_t bound_stride, double* x, int* status, int* iterations,
                               unsigned flags, void* stream)
{
    return batched_box_qp_entry<16, double>(settings, count, n, P, q, l, u, bound_stride, x, status, iterations, flags, stream);
}

int mir_lsq_batched_posvx16_d(size_t count, size_t n, const double* P, const double* rhs, double* x, int* info, void* stream)
{
    return batched_posvx16_entry<double>(count, n, P, rhs, x, info, stream);
}

}  // extern "C"
