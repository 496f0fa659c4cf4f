// boxqp_wave_launch.h -- host side of the batched box-constrained QP solves of order 17 .. 64 (boxqp_wave.h): argument checks,
// the choice of the instance by n (W = 32: n <= 32, two problems a wave; W = 64 above, one), the dynamic LDS of that instance
// (its limit raised first when it is above 48 KB) and the launch. launch_boxqp64_s.hip and launch_boxqp64_d.hip instantiate it
// for float and double, a translation unit each; boxqp_launch.h and its three units are not involved.
#pragma once

#include "boxqp_launch.h"
#include "boxqp_wave.h"

namespace mirlsq {

template <int W, class T> bool boxqp_wave_launch(const BoxQpWaveArgs<T>& a, unsigned max_waves, hipStream_t s)
{
    constexpr size_t lds = boxqp_wave_lds_bytes<W, T>();
    constexpr unsigned per_wave = 64 / W;
    auto kern = k_boxqp_wave<W, T>;
    if (lds > 48 * 1024
        && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return false;
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)a.count + per_wave - 1) / per_wave, max_waves);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, s, a);
    return hipGetLastError() == hipSuccess;
}

// max_waves: the grid's cap (0: kBoxQpMaxWaves of boxqp_launch.h); with 1 one wave solves every problem in sequence
template <class T, class QS>
int batched_box_qp_wave_entry(const QS* settings, size_t count, size_t n, const T* P, const T* q, const T* l, const T* u,
                              size_t bound_stride, T* x, int* status, int* iterations, unsigned flags, void* stream, unsigned max_waves)
{
    if (!settings || !P || !q || !l || !u || !x || !status || n < kBoxQpWaveMinOrder || n > kBoxQpWaveMaxOrder
        || (bound_stride != 0 && bound_stride != n) || count > ((size_t)1 << 30))
        return -1;
    if (count == 0) return 0;
    if (!device_available()) return -5;
    BoxQpWaveArgs<T> a{};
    a.P = P; a.q = q; a.l = l; a.u = u; a.x = x; a.status = status; a.iterations = iterations;
    a.count = (int)count; a.n = (int)n; a.bound_stride = (int)bound_stride;
    a.relTolerance = settings->relTolerance; a.absTolerance = settings->absTolerance; a.maxIterations = settings->maxIterations;
    a.flags = flags;
    const unsigned cap = max_waves ? max_waves : kBoxQpMaxWaves;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool ok = n <= 32 ? boxqp_wave_launch<32, T>(a, cap, s) : boxqp_wave_launch<64, T>(a, cap, s);
    return ok ? 0 : -5;
}

}  // namespace mirlsq
