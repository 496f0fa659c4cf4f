// boxqp_launch.h -- host side of the batched box-constrained QP solves of both layouts (boxqp_rows.h: W = 8, n = 1 .. 8;
// boxqp_rows16.h: W = 16, n = 9 .. 16): argument checks and the dispatch over the eight orders of a layout for one value type.
// launch_boxqp.hip instantiates the 8-wide entry for float and double; launch_boxqp16_s.hip and launch_boxqp16_d.hip the
// 16-wide ones, a translation unit each, so that the parallel build overlaps the two sets of eight kernels.
#pragma once

#include "boxqp_rows16.h"
#include "driver.h"

namespace mirlsq {

// f(IntC<n>) for the run-time n in W - 7 .. W (the caller has checked the range)
template <int W, class F> void boxqp_dispatch(size_t n, F&& f)
{
    switch ((int)n - (W - 7)) {
    case 0: f(IntC<W - 7>{}); break;
    case 1: f(IntC<W - 6>{}); break;
    case 2: f(IntC<W - 5>{}); break;
    case 3: f(IntC<W - 4>{}); break;
    case 4: f(IntC<W - 3>{}); break;
    case 5: f(IntC<W - 2>{}); break;
    case 6: f(IntC<W - 1>{}); break;
    default: f(IntC<W>{}); break;
    }
}

// a wave takes four problems; the grid-stride loop takes the rest (8192 waves: 8 a SIMD on 256 compute units, more than any
// instance keeps resident)
constexpr unsigned kBoxQpMaxWaves = 8192;

template <int W, class T, class QS>
int batched_box_qp_entry(const QS* settings, size_t count, size_t n, const T* P, const T* q, const T* l, const T* u,
                         size_t bound_stride, T* x, int* status, int* iterations, unsigned flags, void* stream)
{
    static_assert(W == 8 || W == 16, "the 8-wide layout of boxqp_rows.h or the 16-wide one of boxqp_rows16.h");
    if (!settings || !P || !q || !l || !u || !x || !status || n < (size_t)(W - 7) || n > (size_t)W
        || (bound_stride != 0 && bound_stride != (size_t)W) || count > ((size_t)1 << 30))
        return -1;
    if (count == 0) return 0;
    if (!device_available()) return -5;
    BoxQpRowsArgs<T> a{};
    a.P = P; a.q = q; a.l = l; a.u = u; a.x = x; a.status = status; a.iterations = iterations;
    a.count = (int)count; a.bound_stride = (int)bound_stride;
    a.relTolerance = settings->relTolerance; a.absTolerance = settings->absTolerance; a.maxIterations = settings->maxIterations;
    a.flags = flags;
    const unsigned blocks = (unsigned)std::min<size_t>((count + 3) / 4, kBoxQpMaxWaves);
    hipStream_t s = static_cast<hipStream_t>(stream);
    boxqp_dispatch<W>(n, [&](auto NC) {
        constexpr int N = decltype(NC)::value;
        if constexpr (W == 8) hipLaunchKernelGGL((k_boxqp_rows<N, T>), dim3(blocks), dim3(64), 0, s, a);
        else hipLaunchKernelGGL((k_boxqp_rows16<N, T>), dim3(blocks), dim3(64), 0, s, a);
    });
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

template <class T>
int batched_posvx16_entry(size_t count, size_t n, const T* P, const T* rhs, T* x, int* info, void* stream)
{
    if (!P || !rhs || !x || !info || n < 9 || n > 16 || count > ((size_t)1 << 30)) return -1;
    if (count == 0) return 0;
    if (!device_available()) return -2;
    const unsigned blocks = (unsigned)std::min<size_t>((count + 3) / 4, kBoxQpMaxWaves);
    hipStream_t s = static_cast<hipStream_t>(stream);
    boxqp_dispatch<kW16>(n, [&](auto NC) {
        hipLaunchKernelGGL((k_posvx_rows16<decltype(NC)::value, T>), dim3(blocks), dim3(64), 0, s, P, rhs, (int)count, x, info);
    });
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace mirlsq
