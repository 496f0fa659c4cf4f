// batched_predict.h -- the fitted curve of a batch of problems on a grid of abscissae of the caller's choice, and its 1-sigma
// confidence band: per problem k and query tq_i
//     value = eval(tq_i; x_k)                       always written: a pure function of x, whatever a fit's status was
//     sigma = sqrt(max(0, g^T C_k g)),  g = d eval / d x at tq_i,  C_k the covariance of the parameters (count x n x n, as
//                                       k_batched_covariance / k_batched16_covariance write it)
// -- the eval_uncertainty of a curve-fit front end, with the model, its derivative and the finite-difference rule that built C
// stated once, in the library. ONE kernel template serves both model widths (1 <= n <= 8 in float or double, 9 <= n <= 16 in
// double); it has nothing of the row-per-lane layouts of the fit kernels:
//   * a wavefront (= a workgroup) works on ONE problem; lane i owns queries i, i + 64, ... : one query per lane and chunk of 64;
//   * the grid is (count, chunks of q) with a stride over the chunks, so any q < 2^31 runs and gridDim.y stays small;
//   * x_k and the problem's box are read through wave-uniform addresses before the first store (scalar loads); C_k is fetched
//     ONCE per wave by one coalesced load, element e by lane e (& 63), the elements of a fixed parameter's row and column under a
//     false predicate -- they are not read -- and then
//       - n^2 values of at most 64 dwords (float at any n <= 8, double at n <= 5): broadcast out of the lanes (v_readlane) into
//         wave-uniform registers,
//       - otherwise (double at n = 6 .. 16): staged in a static LDS array of n^2 values (2 KB at n = 16) and read back through
//         uniform addresses (a broadcast ds_read). The alternative, re-reading C through uniform global loads in the query loop,
//         was compiled too: profiles/r25/batched_predict.txt has the registers of both;
//   * no dynamic LDS, no scratch, no barrier (one wave: wave_lds_fence()).
// The gradient is formed exactly as the covariance kernels form a Jacobian row, without weights and data: Model::grad with
// kBatchedAnalytic, else  g_j = (eval(x with x_j := min(x_j + eps, u_j)) - eval(x with x_j := max(x_j - eps, l_j))) inv_j,
// inv_j = 1 / twh_j or 0 when twh_j == 0. The basis values of a query are computed in registers (Model::basis(tq_i)): the fit's
// per-row table belongs to the fit's t. A parameter with l_j == u_j is FIXED: g_j = 0 and index j takes no part in the form.
//     sigma^2 = sum_j g_j (sum_k C_jk g_k)   over the free indices, k ascending inside, j ascending outside, every multiply-add
// ONE fused operation: reproducible bit for bit. A free diagonal entry C_jj that is not finite (the first in j) IS every sigma of
// the problem: +inf from a degenerate covariance, NaN from a failed fit. All parameters fixed: sigma = 0.
#pragma once

#include "batched16_kernel.h"

namespace mirlsq {

template <class T> struct BatchedPredictArgs {
    T jacobianEpsilon;
    int count, q;
    const T* x;            // count x n
    const T* lower;        // nullptr (with upper: unbounded, nothing fixed), n values (b_stride 0) or count x n (b_stride n)
    const T* upper;
    int b_stride;
    const T* tq;           // q (tq_stride 0) or count x q (tq_stride q)
    int tq_stride;
    uint32_t variant;      // kBatchedAnalytic
    const T* cov;          // count x n x n; read when sigma is wanted
    T* value;              // count x q
    T* sigma;              // count x q, or nullptr: not wanted
};

// where the wave keeps C: in wave-uniform registers while n^2 values are at most 64 dwords, else in static LDS
template <class Model> constexpr bool batched_predict_stages_c()
{
    return (size_t)Model::n * Model::n * sizeof(batched_value_t<Model>) > 64 * 4;
}

template <class Model>
__global__ __launch_bounds__(64) void k_batched_predict(BatchedPredictArgs<batched_value_t<Model>> a)
{
#pragma clang fp contract(off)
    using T = batched_value_t<Model>;
    constexpr int N = Model::n, NB = Model::nb, W = N <= kBatchedNMax ? kBatchedNMax : kW16;
    constexpr bool STAGE = batched_predict_stages_c<Model>();
    constexpr bool HAS_GRAD = batched_has_grad<Model>::value;
    static_assert(N >= 1 && N <= kBatched16NMax, "1 <= n <= 16");
    __shared__ T Cs[STAGE ? N * N : 1];
    const int lane = threadIdx.x, prob = blockIdx.x;
    const bool want = a.sigma != nullptr, boxed = a.lower != nullptr;
    const bool use_g = HAS_GRAD && (a.variant & kBatchedAnalytic) != 0;

    // ---- wave-uniform: the parameters, the two points of every difference, the fixed set
    T x[W], xph[W], xmh[W], inv[W];
    unsigned fix = 0;                                     // bit j: l_j == u_j, parameter j is fixed
#pragma unroll
    for (int j = 0; j < W; ++j) {
        x[j] = j < N ? a.x[(size_t)prob * N + j] : T(0);
        T lo = -Lim<T>::inf(), up = Lim<T>::inf();
        if (boxed && j < N) { lo = a.lower[(size_t)prob * a.b_stride + j]; up = a.upper[(size_t)prob * a.b_stride + j]; }
        const bool fixed_j = j < N && lo == up;
        fix |= fixed_j ? 1u << j : 0u;
        xmh[j] = vmax(x[j] - a.jacobianEpsilon, lo);
        xph[j] = vmin(x[j] + a.jacobianEpsilon, up);
        const T twh = xph[j] - xmh[j];
        inv[j] = (twh != 0 && !fixed_j) ? T(1) / twh : T(0);          // 0: no derivative is formed for a fixed parameter
    }

    // ---- C of the problem, once per wave: element e by lane e & 63, nothing of a fixed parameter's row or column
    T creg[STAGE ? 1 : N * N];
    bool poisoned = false;                                // a free C_jj is not finite: `poison` is every sigma of the problem
    T poison = 0;
    if (want) {
        const T* cp = a.cov + (size_t)prob * N * N;
        if constexpr (STAGE) {
#pragma unroll
            for (int e0 = 0; e0 < N * N; e0 += kWave) {
                const int e = e0 + lane, ej = e / N, ek = e - ej * N;
                if (e < N * N) Cs[e] = (((fix >> ej) | (fix >> ek)) & 1u) ? T(0) : cp[e];
            }
            wave_lds_fence();
        } else {
            const int ej = lane / N, ek = lane - ej * N;
            T mine = 0;
            if (lane < N * N && !(((fix >> ej) | (fix >> ek)) & 1u)) mine = cp[lane];
#pragma unroll
            for (int e = 0; e < N * N; ++e) creg[e] = lane_get(mine, e);
        }
#pragma unroll
        for (int j = N - 1; j >= 0; --j) {                // descending, so that the first in j stays
            T d;
            if constexpr (STAGE) d = Cs[j * N + j]; else d = creg[j * N + j];
            const bool bad = !((fix >> j) & 1u) && !(vabs(d) < Lim<T>::inf());
            poisoned = poisoned || bad;
            poison = bad ? d : poison;
        }
    }

    const T* tp = a.tq + (size_t)prob * a.tq_stride;
    T* vp = a.value + (size_t)prob * a.q;
    T* sp = want ? a.sigma + (size_t)prob * a.q : nullptr;
    const int chunks = (a.q + kWave - 1) / kWave;
    for (int c = blockIdx.y; c < chunks; c += gridDim.y) {
        if constexpr (STAGE) asm volatile("" ::: "memory");           // C stays in LDS: its reads are not hoisted out of this loop
        const int i = c * kWave + lane;
        const bool live = i < a.q;
        const T ti = tp[live ? i : a.q - 1];
        T b[NB > 0 ? NB : 1];
        Model::basis(ti, b);
        const T v = Model::eval(ti, b, x);
        if (live) vp[i] = v;
        if (!want) continue;
        T g[W];
#pragma unroll
        for (int j = 0; j < W; ++j) g[j] = 0;
        if (use_g) {
            if constexpr (HAS_GRAD) {
                Model::grad(ti, b, x, g);
#pragma unroll
                for (int j = 0; j < N; ++j) g[j] = ((fix >> j) & 1u) ? T(0) : g[j];
            }
        } else {
            T p[W];
#pragma unroll
            for (int k = 0; k < W; ++k) p[k] = x[k];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                p[j] = xph[j];
                const T fp = Model::eval(ti, b, p);
                p[j] = xmh[j];
                const T fm = Model::eval(ti, b, p);
                p[j] = x[j];
                const T d = fp - fm;
                g[j] = inv[j] != 0 ? d * inv[j] : T(0);
            }
        }
        T s = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            T inner = 0;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                T cjk;
                if constexpr (STAGE) cjk = Cs[j * N + k]; else cjk = creg[j * N + k];
                inner = ((fix >> k) & 1u) ? inner : __builtin_elementwise_fma(cjk, g[k], inner);
            }
            s = ((fix >> j) & 1u) ? s : __builtin_elementwise_fma(g[j], inner, s);
        }
        const T sg = s > 0 ? vsqrt(s) : (s == s ? T(0) : s);          // sqrt(max(0, s)); a NaN stays one
        if (live) sp[i] = poisoned ? poison : sg;
    }
}

}  // namespace mirlsq
