// launch_boxqp.hip -- batched box-constrained QP solves, four problems a wave (boxqp_rows.h): the sixteen instances of
// k_boxqp_rows (n = 1 .. 8, float and double) and their extern "C" entries mir_lsq_batched_box_qp_s / _d (boxqp_launch.h). A
// translation unit of its own: the units that hold k_lm_batched (batched.hip, batched_d.hip) neither recompile nor grow with it.
#include "boxqp_launch.h"

using namespace mirlsq;

extern "C" {

int mir_lsq_batched_box_qp_s(const mir_box_qp_settings_s* settings, size_t count, size_t n, const float* P, const float* q,
                             const float* l, const float* u, size_t bound_stride, float* x, int* status, int* iterations,
                             unsigned flags, void* stream)
{
    return batched_box_qp_entry<8, float>(settings, count, n, P, q, l, u, bound_stride, x, status, iterations, flags, stream);
}

int mir_lsq_batched_box_qp_d(const mir_box_qp_settings_d* settings, size_t count, size_t n, const double* P, const double* q,
                             const double* l, const double* u, size_t bound_stride, double* x, int* status, int* iterations,
                             unsigned flags, void* stream)
{
    return batched_box_qp_entry<8, double>(settings, count, n, P, q, l, u, bound_stride, x, status, iterations, flags, stream);
}

}  // extern "C"
