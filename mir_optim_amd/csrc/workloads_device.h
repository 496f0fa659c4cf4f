// workloads_device.h -- device helpers shared by the workload translation units (workloads.hip, workloads_gemm.hip):
// DPP lane moves, the compile-time loop, and the tanh / exp the synthetic residuals evaluate (ONE definition: the single-point
// and the batched kernels must round alike).
#pragma once

#include <hip/hip_runtime.h>
#include <omp.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <type_traits>

namespace {


template <int N> __device__ inline int dpp_row_ror(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x120 + N, 0xF, 0xF, false); }
template <int N> __device__ inline double dpp_row_ror(double v)
{
    return __hiloint2double(dpp_row_ror<N>(__double2hiint(v)), dpp_row_ror<N>(__double2loint(v)));
}
template <int N> __device__ inline float dpp_row_ror(float v) { return __int_as_float(dpp_row_ror<N>(__float_as_int(v))); }
// sum over the 16 lanes of a row (DPP row rotations: VALU lane moves, not LDS permutes)
template <typename T> __device__ inline T sum16(T v)
{
    v += dpp_row_ror<8>(v);
    v += dpp_row_ror<4>(v);
    v += dpp_row_ror<2>(v);
    v += dpp_row_ror<1>(v);
    return v;
}

// compile-time loop: f(integral_constant<int, 0>{}), ..., f(integral_constant<int, N - 1>{})
template <int N, typename F, int I = 0> __device__ __forceinline__ void wl_static_for(F&& f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        wl_static_for<N, F, I + 1>(static_cast<F&&>(f));
    }
}

// the value of the neighbouring lane (lane ^ 1): DPP quad_perm [1, 0, 3, 2]
__device__ inline double lane_pair_swap(double v)
{
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0xB1, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0xB1, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}

// tanh for the synthetic residuals: 1 - 2 / (exp(2|x|) + 1) with a degree-13 exp polynomial and a Newton-refined
// reciprocal, ~35 fp64 instructions instead of libm's ~135 (absolute error ~2e-16; the residual tanh(.) - b only
// needs absolute accuracy). The same function is used by the single-point and the batched kernels.
// Held to a long-double tanh within 2^-51 over the whole line by tests/test_gpu_tanh_cells.py (wl_unary_d runs it alone); odd,
// |y| <= 1, +-1 exactly from |x| = 20 on, +-0 kept.
// A NaN DOES NOT COME OUT A NaN: fmin returns the operand that is a number, so dtanh(NaN) = copysign(1, NaN) = +-1, and a NaN in
// x or in A gives a finite residual (libm's tanh, the host callback and the oracle return NaN). A clamp that a NaN passes,
// `t > 40 ? 40 : t` or `2 (ax > 20 ? 20 : ax)`, costs the forked n = 128 difference-panel kernel, which sits at its 168-register
// limit, 12 bytes of scratch memory it does not have today (profiles/r23/dtanh_nan_resources.txt), so the clamp stays as it is:
// a caller who needs a NaN to surface checks x before the call. DESIGN section 11.
__device__ inline double dtanh(double x)
{
    const double ax = fabs(x);
    const double t = fmin(2.0 * ax, 40.0);
    const double kf = rint(t * 1.4426950408889634);
    double r = fma(kf, -6.93147180369123816490e-01, t);
    r = fma(kf, -1.90821492927058770002e-10, r);
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    const double e = ldexp(p, (int)kf);
    const double d = e + 1.0;
    double q = __builtin_amdgcn_rcp(d);
    q = fma(fma(-d, q, 1.0), q, q);
    q = fma(fma(-d, q, 1.0), q, q);
    return copysign(fma(-2.0, q, 1.0), x);
}
__device__ inline float dtanh(float v) { return tanhf(v); }

// The row sum of the tanh-linear residual as the one-point sweep forms it (k_tanh_linear, workloads.hip): 16 lanes per row, lane p
// holds the column pairs (32 c + 2 p, 32 c + 2 p + 1), c < NCP; this is the lane's share, sum16() then adds the 16 lanes.
// ONE definition with the operations written out -- per pair one multiply and one fused multiply-add, t = fma(v0, x0, v1 x1), then
// s = (0 + t_0) + t_1 + ... in c order: the sequence the compiler's contraction used to pick for `s += v0 x0 + v1 x1` in every
// instance of that kernel. The difference-panel GEMM evaluates the extra point of fbRowMajorDiff (p = 2n + 1) with it from its
// LDS image of A, and that residual has to be the sweep's bit for bit; left to contraction, two call sites may round differently.
// (s: the sum over the pairs before these, for a caller that takes the row in pieces.)
template <typename T, int NCP>
__device__ __forceinline__ T tanh_linear_row_sum(const T (&v0)[NCP], const T (&v1)[NCP], const T (&x0)[NCP], const T (&x1)[NCP],
                                                 T s = T(0))
{
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < NCP; ++c) {
        const T hi = v1[c] * x1[c];
        const T t = fma(v0[c], x0[c], hi);
        s = s + t;
    }
    return s;
}
__device__ inline double dexp(double v) { return exp(v); }
__device__ inline float dexp(float v) { return expf(v); }


}  // namespace
