// boxqp16_launch.h -- host side of the 16-wide batched box-constrained QP solves (boxqp_rows16.h): argument checks and the
// dispatch over n = 9 .. 16 for one value type. launch_boxqp16_s.hip and launch_boxqp16_d.hip instantiate it for float and
// double, a translation unit each, so that the parallel build overlaps the two sets of eight kernels.
#pragma once

#include "boxqp_rows16.h"
#include "driver.h"

namespace mirlsq {

// f(IntC<n>) for the run-time n in 9 .. 16
template <class F> void boxqp16_dispatch(size_t n, F&& f)
{
    switch (n) {
    case 9: f(IntC<9>{}); break;
    case 10: f(IntC<10>{}); break;
    case 11: f(IntC<11>{}); break;
    case 12: f(IntC<12>{}); break;
    case 13: f(IntC<13>{}); break;
    case 14: f(IntC<14>{}); break;
    case 15: f(IntC<15>{}); break;
    default: f(IntC<16>{}); break;
    }
}

// a wave takes four problems; the grid-stride loop takes the rest (as launch_boxqp.hip: 8192 waves, more than any instance
// keeps resident)
constexpr unsigned kBoxQp16MaxWaves = 8192;

template <class T, class QS>
int batched_box_qp16_entry(const QS* settings, size_t count, size_t n, const T* P, const T* q, const T* l, const T* u,
                           size_t bound_stride, T* x, int* status, int* iterations, unsigned flags, void* stream)
{
    if (!settings || !P || !q || !l || !u || !x || !status || n < 9 || n > 16 || (bound_stride != 0 && bound_stride != 16)
        || count > ((size_t)1 << 30))
        return -1;
    if (count == 0) return 0;
    if (!device_available()) return -5;
    BoxQpRows16Args<T> a{};
    a.P = P; a.q = q; a.l = l; a.u = u; a.x = x; a.status = status; a.iterations = iterations;
    a.count = (int)count; a.bound_stride = (int)bound_stride;
    a.relTolerance = settings->relTolerance; a.absTolerance = settings->absTolerance; a.maxIterations = settings->maxIterations;
    a.flags = flags;
    const unsigned blocks = (unsigned)std::min<size_t>((count + 3) / 4, kBoxQp16MaxWaves);
    hipStream_t s = static_cast<hipStream_t>(stream);
    boxqp16_dispatch(n, [&](auto NC) {
        hipLaunchKernelGGL((k_boxqp_rows16<decltype(NC)::value, T>), dim3(blocks), dim3(64), 0, s, a);
    });
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

template <class T>
int batched_posvx16_entry(size_t count, size_t n, const T* P, const T* rhs, T* x, int* info, void* stream)
{
    if (!P || !rhs || !x || !info || n < 9 || n > 16 || count > ((size_t)1 << 30)) return -1;
    if (count == 0) return 0;
    if (!device_available()) return -2;
    const unsigned blocks = (unsigned)std::min<size_t>((count + 3) / 4, kBoxQp16MaxWaves);
    hipStream_t s = static_cast<hipStream_t>(stream);
    boxqp16_dispatch(n, [&](auto NC) {
        hipLaunchKernelGGL((k_posvx_rows16<decltype(NC)::value, T>), dim3(blocks), dim3(64), 0, s, P, rhs, (int)count, x, info);
    });
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace mirlsq
