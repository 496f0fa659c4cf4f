// batched16_kernel.h -- many small independent LM fits with 9 to 16 PARAMETERS, one wavefront per problem, double precision.
// The counterpart of k_lm_batched (batched_kernel.h, n <= 8) at the width of the 16-lane-row solves: the whole loop of
// optimizeLeastSquaresImplGeneric!double (the reference's least_squares.d:877-1176, cited as LS:line) inside one kernel.
//   * a single-wave workgroup owns one problem. Its LDS holds J with a ROW STRIDE OF 16 doubles (columns >= Model::n are
//     zeros), y, the previous / trial residual, and one 16 x 16 J^T J tile with J^T y behind it:
//         (16 + 2) m + 272 doubles;   (16 + 2) 8 m + 2176 <= 160 KB - 512   <=>   m <= 1119       (batched16_lds_bytes)
//   * x[16] is replicated in every lane (components >= n are 0); residual, finite differences / Model::grad and the Broyden
//     update take the rows lane, lane + 64, ... as k_lm_batched does;
//   * J^T J is ONE v_mfma_f64_16x16x4_f64 tile: step s feeds the four rows 4 s .. 4 s + 3 of J; the A and the B operand are
//     the same register, the lane's value J[4 s + (lane >> 4)][lane & 15] (Mma<double>: A[i = l & 15][k = l >> 4] and
//     B[k = l >> 4][j = l & 15] -- A = J^T, B = J), so the 64 lanes read 512 contiguous bytes of LDS per instruction. The
//     accumulator of lane l, register q is element (row (l >> 4) + 4 q, column l & 15). Both triangles sum the same
//     products in the same order: the tile is exactly symmetric. J^T y rides on the loaded value (one fused multiply-add
//     with y broadcast from LDS; the four row-quarters are summed by a butterfly at the end);
//   * the tile goes to LDS, every lane reads row r = lane & 15 back, and wave16_lm_solve<N, true> (solve_wave16.h) does the
//     pass's n x n work with ONE damping value per solve: lambda_0, the damped ?posvx, the BOXCQP active-set loop when the
//     step leaves the box, the rounded step, the trial point, the predicted reduction and the flags. Bounds are always
//     handled here: no problem returns kBatchedNeedsGeneral; a QP that does not end as solved ends its fit with -26;
//   * acceptance, the lambda / mu schedule and the exit tests are the macros of lm_rules.h.
// In the kernel's OWN arithmetic contraction is off and every fused multiply-add is written out, as in batched_kernel.h; the
// pragma is lexical, so a model's eval / grad are compiled as their author wrote them (the two built-in models below set the
// pragma and spell their fused multiply-adds out; a caller's model is the caller's business). Control flow is wave-uniform; lanes
// exchange data through LDS behind wave_lds_fence(), there is no barrier.
// The model contract is that of batched_kernel.h with 9 <= n <= 16, value_type = double and 16 entries in x.
#pragma once

#include "batched_kernel.h"
#include "solve_wave16.h"

namespace mirlsq {

constexpr int kBatched16NMin = 9, kBatched16NMax = 16;
constexpr int kBatched16TileDoubles = kW16 * kW16 + kW16;        // J^T J, then J^T y

enum : int { kModel16ExpHarm16 = 16, kModel16Gauss3Affine = 17 };

// p0 exp(-t p1) + p2 + sum_{j = 3 .. N - 1} p_j h_j(t),  h_j = sin(k w t) (j odd) or cos(k w t) (j even), k = (j - 1) / 2,
// w = pi / 2: the decay of ModelExpDecayPad8D with N - 3 terms that are linear in their parameters (the row's basis).
// N = 16 is the built-in MIR_LSQ_MODEL16_EXP_HARM16 (seven sines and six cosines).
template <int N> struct ModelExpHarm {
    using value_type = double;
    static constexpr int n = N, nb = N - 3;
    __device__ static inline void basis(double t, double* b)
    {
#pragma unroll
        for (int j = 3; j < N; ++j) {
            const double a = (double)((j - 1) / 2) * 1.5707963267948966 * t;
            b[j - 3] = (j & 1) ? sin(a) : cos(a);
        }
    }
    __device__ static inline double eval(double t, const double* b, const double* x)
    {
#pragma clang fp contract(off)
        double v = __builtin_elementwise_fma(x[0], exp(-t * x[1]), x[2]);
#pragma unroll
        for (int j = 3; j < N; ++j) v = __builtin_elementwise_fma(x[j], b[j - 3], v);
        return v;
    }
    __device__ static inline void grad(double t, const double* b, const double* x, double* g)
    {
        const double e = exp(-t * x[1]);
        g[0] = e; g[1] = -t * x[0] * e; g[2] = 1.0;
#pragma unroll
        for (int j = 3; j < N; ++j) g[j] = b[j - 3];
    }
};
using ModelExpHarm16 = ModelExpHarm<16>;

// MIR_LSQ_MODEL16_GAUSS3_AFFINE (n = 11): sum_{k < 3} p_{3k} exp(-((t - p_{3k+1}) / p_{3k+2})^2 / 2) + p9 + p10 t
struct ModelGauss3Affine {
    using value_type = double;
    static constexpr int n = 11, nb = 0;
    __device__ static inline void basis(double, double*) {}
    __device__ static inline double eval(double t, const double*, const double* x)
    {
#pragma clang fp contract(off)
        double v = __builtin_elementwise_fma(x[10], t, x[9]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double z = (t - x[3 * k + 1]) / x[3 * k + 2];
            v = __builtin_elementwise_fma(x[3 * k], exp(-0.5 * (z * z)), v);
        }
        return v;
    }
};

template <int ID> struct BuiltinModel16;
template <> struct BuiltinModel16<kModel16ExpHarm16> { using type = ModelExpHarm16; };
template <> struct BuiltinModel16<kModel16Gauss3Affine> { using type = ModelGauss3Affine; };

// J^T J (16 x 16) and J^T y (16) of the m x 16 LDS-resident J (row stride 16) by ONE wave, written to tile[0 .. 256) and
// tile[256 .. 272). Rows >= m contribute exact zeros (m need not be a multiple of 4; the address is clamped to the last row).
__device__ __forceinline__ void jtj16_tile(const double* Jl, const double* yv, int m, double* tile)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    wave_lds_fence();                                          // J and y were written by other lanes of this wave
    Mma<double>::Acc acc = {0.0, 0.0, 0.0, 0.0};
    double accy = 0.0;
    const int steps = (m + 3) >> 2;
    for (int s = 0; s < steps; ++s) {
        const int row = 4 * s + g, rc = row < m ? row : m - 1;
        const double jv = Jl[(size_t)rc * kW16 + c], yy = yv[rc];
        const double v = row < m ? jv : 0.0, yi = row < m ? yy : 0.0;
        acc = Mma<double>::mma(v, v, acc);
        accy = __builtin_elementwise_fma(v, yi, accy);
    }
    // the four row-quarters of J^T y: (p_g + p_{g ^ 1}) + (p_{g ^ 2} + p_{g ^ 3}), the same bits in every group
    accy += wave_shfl_xor(accy, 16);
    accy += wave_shfl_xor(accy, 32);
#pragma unroll
    for (int q = 0; q < 4; ++q) tile[(g + 4 * q) * kW16 + c] = acc[q];
    if (g == 0) tile[kW16 * kW16 + c] = accy;
    wave_lds_fence();
}

// WEIGHTED: the rules of k_lm_batched (batched_kernel.h) at this width. The residual of row i is w_i (eval - data_i), ONE
// multiplication after the subtraction, wherever a residual or a Jacobian row is formed (feval; each finite-difference point
// before the two are differenced; J_ij = w_i g_j on the analytic path; the Broyden update sees weighted residuals only). The
// weights are read from global memory next to t and data, in the same clamped loads: the LDS and the m limit are unchanged. A
// weight of exactly 0 gives a zero residual and a zero Jacobian row. The unweighted instance does not read a.weights and is,
// instruction for instruction, what it was before the parameter existed.
template <class Model, bool WEIGHTED = false>
__global__ __launch_bounds__(64, 1) void k_lm_batched16(BatchedArgs<double> a)
{
#pragma clang fp contract(off)
    using T = double;
    static_assert(std::is_same<batched_value_t<Model>, double>::value, "k_lm_batched16: value_type = double");
    constexpr int N = Model::n, NB = Model::nb, W = kW16;
    static_assert(N >= kBatched16NMin && N <= kBatched16NMax, "9 <= n <= 16");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    const int lane = threadIdx.x, r = lane & 15, prob = blockIdx.x, m = a.m;
    const bool el = r < N;
    T* Jl = reinterpret_cast<T*>(smem_b);                        // J: m x 16 row-major
    T* yv = Jl + (size_t)W * m;
    T* mB = yv + m;
    T* tile = mB + m;                                            // both residual buffers lie below it: a swap does not move it
    const T* tp = a.t + (size_t)(a.t_stride ? prob : 0) * a.t_stride;
    const T* dp = a.data + (size_t)prob * m;
    const T* bp = NB ? a.basis + (size_t)(a.t_stride ? prob : 0) * a.t_stride * NB : nullptr;
    const LmSettingsDev<T>& S = a.set;
    const T* wp = nullptr;
    if constexpr (WEIGHTED) wp = a.weights + (size_t)(a.w_stride ? prob : 0) * a.w_stride;

    // component r of x and of the bounds in lane r of every 16-lane group; x replicated in every lane beside it
    T xr = a.x[(size_t)prob * N + (el ? r : 0)];
    const size_t bo = (size_t)prob * a.b_stride + (el ? r : 0);   // the problem's own box (b_stride n) or the shared one (0)
    T lo_r = a.lower[bo], up_r = a.upper[bo];
    xr = el ? xr : T(0);
    lo_r = el ? lo_r : -Lim<T>::inf();
    up_r = el ? up_r : Lim<T>::inf();
    T x[W];
    static_for<W>([&](auto K) { constexpr int k = decltype(K)::value; x[k] = dpp_row_bcast<k>(xr); });

    BatchedResult<T> ret;
    ret.status = -26;   // numericError, LS:132
    ret.iterations = 0; ret.fCalls = 0; ret.gCalls = 0;
    ret.residual = Lim<T>::inf(); ret.lambda = 0;

    auto feval = [&](const T (&p)[W], T* dst) -> T {                     // dst = f(p); returns ||f||^2
        constexpr int UNR = NB > 4 ? 2 : 4;
        T ss = 0;
        for (int base = lane; base - lane < m; base += kWave * UNR) {
            T tv[UNR], dv[UNR], rv[UNR], wv[WEIGHTED ? UNR : 1];
            BasisRow<NB, T> bv[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int i = min(base + kWave * u, m - 1);
                tv[u] = tp[i]; dv[u] = dp[i];
                if constexpr (WEIGHTED) wv[u] = wp[i];
                bv[u].load(bp, i);
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                rv[u] = Model::eval(tv[u], bv[u].v, p) - dv[u];
                if constexpr (WEIGHTED) rv[u] = wv[u] * rv[u];
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int i = base + kWave * u;
                if (i < m) dst[i] = rv[u];
                ss = i < m ? __builtin_elementwise_fma(rv[u], rv[u], ss) : ss;
            }
        }
        return wave_sum(ss);
    };

    // validation LS:930-943 (settings were checked on the host; x / bounds here)
    const bool finite = __ballot(el && !(-Lim<T>::inf() < xr && xr < Lim<T>::inf())) == 0;
    const bool inb = __ballot(el && (!(lo_r <= xr) || !(xr <= up_r))) == 0;
    if (m == 0 || !finite) ret.status = -31;           // badGuess
    else if (!inb) ret.status = -32;                   // badBounds
    else {
        constexpr bool HAS_GRAD = batched_has_grad<Model>::value;
        const bool use_g = HAS_GRAD && (a.variant & kBatchedAnalytic) != 0;  // g of LS:1010-1014 (the launcher refuses it without grad)
        const uint32_t maxAge = a.maxAge ? a.maxAge : (use_g ? 3u : 2u * N);     // LS:945
        if constexpr (N < W) {                                             // the padded columns of J are zero once and for all
            for (int i = lane; i < m; i += kWave)
#pragma unroll
                for (int j = N; j < W; ++j) Jl[(size_t)i * W + j] = T(0);
        }
        ret.residual = feval(x, yv);                                       // LS:953-955
        ++ret.fCalls;
        bool fConverged = LM_F_CONVERGED(ret.residual, S);
        bool needJacobian = true;
        uint32_t age = maxAge;
        T dx[W], JJrow[W], djj = 0, Jy_r = 0;
#pragma unroll
        for (int j = 0; j < W; ++j) { dx[j] = 0; JJrow[j] = 0; }
        T dx_dot = 0, mu = 1, lambda = 0;
        ret.status = -1;                                                   // maxIterations, LS:971
        do {
            if (fConverged) { ret.status = 3; break; }                     // LS:974
            if (!LM_LAMBDA_IN_RANGE(lambda, S)) { ret.status = 0; break; } // LS:979
            if (mu > kSuspiciousMu && age) { needJacobian = true; age = maxAge; mu = 1; }   // LS:984
            if (__ballot(el && !(xr <= xr)) != 0) { ret.status = -26; break; }              // LS:990
            bool fresh = false;                                            // J^T y is new: the solve applies LS:1053 first
            if (needJacobian) {                                            // LS:996
                needJacobian = false;
                fresh = true;
                if (age < maxAge) {                                        // Broyden LS:999-1007
                    age++;
                    const T d = T(1) / dx_dot;
                    for (int i = lane; i < m; i += kWave) {
                        T* Ji = Jl + (size_t)i * W;
                        T dot = 0;
#pragma unroll
                        for (int j = 0; j < N; ++j) dot = __builtin_elementwise_fma(Ji[j], dx[j], dot);
                        const T t = (mB[i] - yv[i]) + dot;                 // mB holds the previous residual
                        const T u = -d * t;
#pragma unroll
                        for (int j = 0; j < N; ++j) Ji[j] = __builtin_elementwise_fma(u, dx[j], Ji[j]);
                    }
                } else if (use_g) {                                        // g(x, J), LS:1010-1014
                    age = 0;
                    if constexpr (HAS_GRAD) {
                        for (int i = lane; i < m; i += kWave) {
                            BasisRow<NB, T> b;
                            b.load(bp, i);
                            T gi[W];
#pragma unroll
                            for (int j = 0; j < W; ++j) gi[j] = 0;
                            Model::grad(tp[i], b.v, x, gi);
                            if constexpr (WEIGHTED) {
                                const T wi = wp[i];
#pragma unroll
                                for (int j = 0; j < N; ++j) gi[j] = wi * gi[j];
                            }
#pragma unroll
                            for (int j = 0; j < N; ++j) Jl[(size_t)i * W + j] = gi[j];
                        }
                    }
                    ++ret.gCalls;                                          // LS:1013
                } else {                                                   // FD LS:1016-1050: central, clipped to the box
                    age = 0;
                    const T xmh_r = vmax(xr - S.jacobianEpsilon, lo_r), xph_r = vmin(xr + S.jacobianEpsilon, up_r);
                    const T twh_r = xph_r - xmh_r;
                    const T inv_r = twh_r != 0 ? T(1) / twh_r : T(0);      // a zero-width interval: the column is zero, LS:1045
                    T xph[W], xmh[W], inv[W];
                    static_for<W>([&](auto K) {
                        constexpr int k = decltype(K)::value;
                        xph[k] = dpp_row_bcast<k>(xph_r); xmh[k] = dpp_row_bcast<k>(xmh_r); inv[k] = dpp_row_bcast<k>(inv_r);
                    });
                    for (int i = lane; i < m; i += kWave) {
                        BasisRow<NB, T> b;
                        b.load(bp, i);
                        const T ti = tp[i], di = dp[i];
                        T p[W];
#pragma unroll
                        for (int k = 0; k < W; ++k) p[k] = x[k];
#pragma unroll
                        for (int j = 0; j < N; ++j) {
                            p[j] = xph[j];
                            T fp = Model::eval(ti, b.v, p) - di;
                            if constexpr (WEIGHTED) fp = wp[i] * fp;          // wp[i]: one load a row. (A local for it, declared outside
                            p[j] = xmh[j];
                            T fm = Model::eval(ti, b.v, p) - di;
                            if constexpr (WEIGHTED) fm = wp[i] * fm;          // the branch, reorders two moves of the unweighted instance.)
                            p[j] = x[j];
                            const T v = fp - fm;
                            Jl[(size_t)i * W + j] = inv[j] != 0 ? v * inv[j] : T(0);
                        }
                    }
                    ret.fCalls += N;                                       // LS:1049 (quirk Q5)
                }
                // Jy = J^T y (LS:1052) and JJ = J^T J (LS:1065) on the matrix unit; the lane takes row r of the tile
                jtj16_tile(Jl, yv, m, tile);
#pragma unroll
                for (int k = 0; k < W; ++k) JJrow[k] = tile[r * W + k];
                djj = tile[r * W + r];
                Jy_r = tile[W * W + r];
            }
            // LS:1053-1110 and 1141-1142, 1164: the gradient test of a new J^T y, lambda_0, the box QP of the damped system,
            // the rounded step, the trial point, the predicted reduction. Every group solves the same system; group 0 reports.
            Wave16Level lv;
            T d_r, tr_r;
            wave16_lm_solve<N, true>(JJrow, djj, Jy_r, xr, lo_r, up_r, lambda, mu, fresh, true, S, lv, d_r, tr_r, N, true);
            const int flags = __builtin_amdgcn_readfirstlane(lv.flags);
            if (flags & kFlagGradSmall) {                                  // LS:1053-1062
                if (age == 0) { ret.status = 2; break; }
                age = maxAge;
                continue;
            }
            lambda = lane_bcast(lv.lambda, 0);                             // LS:1067-1072
            if (__builtin_amdgcn_readfirstlane(lv.qp_status) != 0) { ret.status = -26; break; }   // LS:1080-1085
            if (flags & kFlagDxNaN) { ret.status = -26; break; }           // LS:1087
            if (flags & kFlagStepTooLong) { LM_REJECT(lambda, mu, S); continue; }   // LS:1101-1106
            // kFlagXNaN and kFlagNullStep are not read: a NaN trial point gives a NaN trial residual, which LS:1117 below turns
            // into -26, and a null step is evaluated like any other (its improvement is 0: rejected at LS:1125), as in k_lm_batched
            T trial[W], sol[W];
#pragma unroll
            for (int k = 0; k < W; ++k) { trial[k] = lane_bcast(tr_r, k); sol[k] = lane_bcast(d_r, k); }   // group 0's
            ++ret.fCalls;                                                  // LS:1112-1115
            // the trial residual goes to the buffer that is NOT the current y
            const T trialResidual = feval(trial, mB);
            if (!(trialResidual <= Lim<T>::inf())) { ret.status = -26; break; }       // LS:1117
            const T improvement = ret.residual - trialResidual;
            if (!(improvement > 0)) { LM_REJECT(lambda, mu, S); continue; }   // LS:1125-1130
            needJacobian = true;                                           // LS:1132-1139
            mu = 1;
            ret.iterations++;
            xr = T(0);
            static_for<W>([&](auto K) {
                constexpr int k = decltype(K)::value;
                x[k] = trial[k]; dx[k] = sol[k];
                xr = (r == k) ? trial[k] : xr;
            });
            { T* tmp = yv; yv = mB; mB = tmp; }                            // swap(mBuffer, y): mB = previous residual
            ret.residual = trialResidual;
            fConverged = LM_F_CONVERGED(ret.residual, S);
            dx_dot = lane_bcast(lv.ndd, 0);
            const T pred = lane_bcast(lv.pred, 0);                         // LS:1141-1142 (undamped JJ)
            if (!(pred > 0)) { ret.status = 0; break; }                    // LS:1144-1148
            const T rho = pred / improvement;                              // LS:1150 (Q2)
            LM_RATE_STEP(rho, lambda, mu, S);                              // LS:1152-1161
            if (!LM_X_MOVING(vsqrt(dx_dot), lane_bcast(lv.xnorm, 0), S)) { // LS:1164-1173 (Q6)
                if (age == 0) { ret.status = 1; break; }
                age = maxAge;
                continue;
            }
        } while (ret.iterations < a.maxIterations);                        // LS:1175
        ret.lambda = lambda;
    }
    if (lane == 0) a.results[prob] = ret;
    if (lane < N) a.x[(size_t)prob * N + lane] = xr;
}

// ---- covariance of the fitted parameters in the 16-lane layout, one single-wave workgroup per problem -------------------------
// The contract of k_batched_covariance (batched_kernel.h): cov = s^2 (J^T J)^-1, s^2 = ||f(x)||^2 / (rows with a nonzero weight
// - n) or 1 with kBatchedAbsoluteSigma; status and ||f(x)||^2 come from the fit's record. J is rebuilt at the final x into LDS
// as a refresh of k_lm_batched16 builds it (Model::grad with kBatchedAnalytic, else central differences with jacobianEpsilon
// clipped to the bounds; weighted rows; row stride 16, padded columns zero), J^T J is the jtj16_tile of the fit, and the inverse
// is posvx_rows16<N> without a shift on unit right-hand sides: the four 16-lane groups take four columns a call. The columns
// meet in LDS (where the tile was), and element (i, c) is s^2 (v_ic + v_ci) / 2: symmetric bit for bit. n x n values a problem,
// row-major. Degenerate cases:
//     status < 0                                                        every entry NaN
//     a non-positive pivot in the factorization, or rows - n_free <= 0   every free entry +inf
// The box is the problem's own (BatchedCovArgs::b_stride n) or the shared one (0). A parameter with l_j == u_j in it is FIXED,
// as in k_batched_covariance: its column of J is zero, its row is not a live row
// of posvx_rows16 (identity row and column: the system solved is the reduced one, of order n_free), row j and column j of the
// result are exactly 0, and s^2 divides by rows - n_free. Without a fixed parameter every operation is the one it was.
// LDS: J, one m-vector of zeros where jtj16_tile reads y, the tile: (16 + 1) m + 272 doubles -- less than the fit's.
// Control flow is wave-uniform; lanes exchange data through LDS behind wave_lds_fence(), there is no barrier.
template <class Model>
__global__ __launch_bounds__(64, 1) void k_batched16_covariance(BatchedCovArgs<double> a)
{
#pragma clang fp contract(off)
    using T = double;
    static_assert(std::is_same<batched_value_t<Model>, double>::value, "k_batched16_covariance: value_type = double");
    constexpr int N = Model::n, NB = Model::nb, W = kW16;
    static_assert(N >= kBatched16NMin && N <= kBatched16NMax, "9 <= n <= 16");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4, prob = blockIdx.x, m = a.m;
    const bool el = r < N;
    T* out = a.cov + (size_t)prob * N * N;
    if (a.results[prob].status < 0) {
        for (int idx = lane; idx < N * N; idx += kWave) out[idx] = Lim<T>::inf() - Lim<T>::inf();   // NaN
        return;
    }
    T* Jl = reinterpret_cast<T*>(smem_b);                        // J: m x 16 row-major
    T* yv = Jl + (size_t)W * m;
    T* tile = yv + m;
    const T* tp = a.t + (size_t)(a.t_stride ? prob : 0) * a.t_stride;
    const T* dp = a.data + (size_t)prob * m;
    const T* bp = NB ? a.basis + (size_t)(a.t_stride ? prob : 0) * a.t_stride * NB : nullptr;
    const T* wp = a.weights ? a.weights + (size_t)(a.w_stride ? prob : 0) * a.w_stride : nullptr;

    T xr = a.x[(size_t)prob * N + (el ? r : 0)];
    const size_t bo = (size_t)prob * a.b_stride + (el ? r : 0);   // the problem's own box (b_stride n) or the shared one (0)
    T lo_r = a.lower[bo], up_r = a.upper[bo];
    xr = el ? xr : T(0);
    lo_r = el ? lo_r : -Lim<T>::inf();
    up_r = el ? up_r : Lim<T>::inf();
    T x[W];
    static_for<W>([&](auto K) { constexpr int k = decltype(K)::value; x[k] = dpp_row_bcast<k>(xr); });
    // l_j == u_j: parameter j is fixed. Bit j of `fix` (wave-uniform); free_r: row r belongs to the system that is solved
    const bool fixed_r = el && lo_r == up_r;
    const unsigned fix = (unsigned)(__ballot(fixed_r) & 0xffffull);
    const bool free_r = el && !fixed_r;
    const int nfree = N - __builtin_popcount(fix);

    constexpr bool HAS_GRAD = batched_has_grad<Model>::value;
    const bool use_g = HAS_GRAD && (a.variant & kBatchedAnalytic) != 0;
    T rows = 0;
    if (use_g) {
        if constexpr (HAS_GRAD) {
            for (int i = lane; i < m; i += kWave) {
                BasisRow<NB, T> b;
                b.load(bp, i);
                const T wi = wp ? wp[i] : T(1);
                rows += wi != 0 ? T(1) : T(0);
                T gi[W];
#pragma unroll
                for (int j = 0; j < W; ++j) gi[j] = 0;
                Model::grad(tp[i], b.v, x, gi);
                if (wp) {
#pragma unroll
                    for (int j = 0; j < N; ++j) gi[j] = wi * gi[j];
                }
#pragma unroll
                for (int j = 0; j < W; ++j) Jl[(size_t)i * W + j] = (j < N && !((fix >> j) & 1u)) ? gi[j] : T(0);   // no column for a fixed one
                yv[i] = T(0);
            }
        }
    } else {
        const T xmh_r = vmax(xr - a.jacobianEpsilon, lo_r), xph_r = vmin(xr + a.jacobianEpsilon, up_r);
        const T twh_r = xph_r - xmh_r;
        const T inv_r = (twh_r != 0 && !fixed_r) ? T(1) / twh_r : T(0);     // 0: the column is not formed
        T xph[W], xmh[W], inv[W];
        static_for<W>([&](auto K) {
            constexpr int k = decltype(K)::value;
            xph[k] = dpp_row_bcast<k>(xph_r); xmh[k] = dpp_row_bcast<k>(xmh_r); inv[k] = dpp_row_bcast<k>(inv_r);
        });
        for (int i = lane; i < m; i += kWave) {
            BasisRow<NB, T> b;
            b.load(bp, i);
            const T ti = tp[i], di = dp[i], wi = wp ? wp[i] : T(1);
            rows += wi != 0 ? T(1) : T(0);
            T p[W];
#pragma unroll
            for (int k = 0; k < W; ++k) p[k] = x[k];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                p[j] = xph[j];
                T fp = Model::eval(ti, b.v, p) - di;
                p[j] = xmh[j];
                T fm = Model::eval(ti, b.v, p) - di;
                p[j] = x[j];
                if (wp) { fp = wi * fp; fm = wi * fm; }
                const T v = fp - fm;
                Jl[(size_t)i * W + j] = inv[j] != 0 ? v * inv[j] : T(0);
            }
#pragma unroll
            for (int j = N; j < W; ++j) Jl[(size_t)i * W + j] = T(0);
            yv[i] = T(0);
        }
    }
    const T dof = wave_sum(rows) - T(nfree);              // row counts are small integers: exact
    jtj16_tile(Jl, yv, m, tile);
    T JJrow[W];
#pragma unroll
    for (int k = 0; k < W; ++k) JJrow[k] = tile[r * W + k];
    const T djj = tile[r * W + r];
    wave_lds_fence();                                     // every lane holds its row: the tile now takes the inverse
    // column c = 4 q + g of the inverse by group g: the right-hand side is the unit vector e_c (zero for c >= N: not read)
    int info = 0;
#pragma nounroll
    for (int q = 0; q < (N + 3) / 4; ++q) {
        const int c = 4 * q + g;
        T v_r;
        // the rows of fixed parameters are not live: identity rows and columns, a zero right-hand side, a zero solution
        info |= posvx_rows16<N>(JJrow, 0.0, djj, (r == c && free_r) ? T(1) : T(0), free_r, r, v_r, nfree);
        tile[r * W + c] = v_r;                            // c <= 15
    }
    info = __builtin_amdgcn_readfirstlane(info);          // the four groups factor the same matrix
    wave_lds_fence();
    const T s2 = (a.flags & kBatchedAbsoluteSigma) ? T(1) : a.results[prob].residual / dof;
    const bool degenerate = info != 0 || !(dof > 0);
    for (int idx = lane; idx < N * N; idx += kWave) {
        const int i = idx / N, c = idx - i * N;
        const T v = s2 * ((tile[i * W + c] + tile[c * W + i]) / 2);
        const bool fx = (((fix >> i) | (fix >> c)) & 1u) != 0;          // row and column of a fixed parameter: exactly 0
        out[idx] = fx ? T(0) : (degenerate ? Lim<T>::inf() : v);
    }
}

// unit entry of jtj16_tile (mir_lsq_batched16_jtj_d): J count x m x n and y count x m in global memory, one wave per problem;
// JJ count x 16 x 16 and Jy count x 16 out. LDS: 17 m + 272 doubles. (A template, so that only the unit that launches it holds it.)
template <int W = kW16>
__global__ __launch_bounds__(64) void k_batched16_jtj(int count, int m, int n, const double* __restrict__ J, const double* __restrict__ y,
                                                      double* __restrict__ JJ, double* __restrict__ Jy)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    const int lane = threadIdx.x, prob = blockIdx.x;
    if (prob >= count) return;
    double* Jl = reinterpret_cast<double*>(smem_b);
    double* yv = Jl + (size_t)kW16 * m;
    double* tile = yv + m;
    for (int idx = lane; idx < m * kW16; idx += kWave) {
        const int i = idx >> 4, j = idx & 15;
        Jl[idx] = j < n ? J[((size_t)prob * m + i) * n + j] : 0.0;
    }
    for (int i = lane; i < m; i += kWave) yv[i] = y[(size_t)prob * m + i];
    jtj16_tile(Jl, yv, m, tile);
    for (int idx = lane; idx < kW16 * kW16; idx += kWave) JJ[(size_t)prob * kW16 * kW16 + idx] = tile[idx];
    if (lane < kW16) Jy[(size_t)prob * kW16 + lane] = tile[kW16 * kW16 + lane];
}

}  // namespace mirlsq
