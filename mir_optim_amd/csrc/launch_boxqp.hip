// launch_boxqp.hip -- batched box-constrained QP solves, four problems a wave (boxqp_rows.h): the sixteen instances of
// k_boxqp_rows (n = 1 .. 8, float and double) and their extern "C" entries mir_lsq_batched_box_qp_s / _d. A translation unit of
// its own: the units that hold k_lm_batched (batched.hip, batched_d.hip) neither recompile nor grow with it.
#include "boxqp_rows.h"
#include "driver.h"

using namespace mirlsq;

namespace {

template <int N, class T>
void boxqp_launch(const BoxQpRowsArgs<T>& a, unsigned blocks, hipStream_t s)
{
    hipLaunchKernelGGL((k_boxqp_rows<N, T>), dim3(blocks), dim3(64), 0, s, a);
}

template <class T, class QS>
int batched_box_qp_entry(const QS* settings, size_t count, size_t n, const T* P, const T* q, const T* l, const T* u,
                         size_t bound_stride, T* x, int* status, int* iterations, unsigned flags, void* stream)
{
    if (!settings || !P || !q || !l || !u || !x || !status || n < 1 || n > 8 || (bound_stride != 0 && bound_stride != 8)
        || count > ((size_t)1 << 30))
        return -1;
    if (count == 0) return 0;
    if (!device_available()) return -5;
    BoxQpRowsArgs<T> a{};
    a.P = P; a.q = q; a.l = l; a.u = u; a.x = x; a.status = status; a.iterations = iterations;
    a.count = (int)count; a.bound_stride = (int)bound_stride;
    a.relTolerance = settings->relTolerance; a.absTolerance = settings->absTolerance; a.maxIterations = settings->maxIterations;
    a.flags = flags;
    // a wave takes four problems; the grid-stride loop takes the rest (8192 waves: 8 a SIMD on 256 compute units, more than any
    // instance keeps resident)
    const unsigned blocks = (unsigned)std::min<size_t>((count + 3) / 4, 8192);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (n) {
    case 1: boxqp_launch<1, T>(a, blocks, s); break;
    case 2: boxqp_launch<2, T>(a, blocks, s); break;
    case 3: boxqp_launch<3, T>(a, blocks, s); break;
    case 4: boxqp_launch<4, T>(a, blocks, s); break;
    case 5: boxqp_launch<5, T>(a, blocks, s); break;
    case 6: boxqp_launch<6, T>(a, blocks, s); break;
    case 7: boxqp_launch<7, T>(a, blocks, s); break;
    default: boxqp_launch<8, T>(a, blocks, s); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace

extern "C" {

int mir_lsq_batched_box_qp_s(const mir_box_qp_settings_s* settings, size_t count, size_t n, const float* P, const float* q,
                             const float* l, const float* u, size_t bound_stride, float* x, int* status, int* iterations,
                             unsigned flags, void* stream)
{
    return batched_box_qp_entry<float>(settings, count, n, P, q, l, u, bound_stride, x, status, iterations, flags, stream);
}

int mir_lsq_batched_box_qp_d(const mir_box_qp_settings_d* settings, size_t count, size_t n, const double* P, const double* q,
                             const double* l, const double* u, size_t bound_stride, double* x, int* status, int* iterations,
                             unsigned flags, void* stream)
{
    return batched_box_qp_entry<double>(settings, count, n, P, q, l, u, bound_stride, x, status, iterations, flags, stream);
}

}  // extern "C"
