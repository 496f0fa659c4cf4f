// boxqp_wave.h -- solveBoxQP (the reference's mir/optim/boxcqp.d:122-379, cited as QP:) for orders 17 .. 64, the order a
// RUN-TIME argument: k_boxqp_wave<W, T>, W = 32 (n <= 32, TWO problems a wave: lanes 0..31 and 32..63) or W = 64 (n = 33 .. 64,
// one problem a wave), T float or double -- four instances in all. The DPP-row layouts of boxqp_rows.h / boxqp_rows16.h stop at
// sixteen lanes a row and keep the matrices in registers (384 f64 registers a lane at n = 64); here they live in LDS:
//   * lane r = lane & (W - 1) of a problem ("half" h = lane / W) owns row r of every matrix and component r of every vector;
//   * the symmetrised P and the Cholesky factor F are W x W in LDS with the row stride S = W + 1 (odd: a lane walking its own
//     row while all lanes read the same column index touches W different banks, and a read of one address by all lanes is a
//     broadcast); the upper triangle of F is written as zeros, so every word a problem reads was written for that problem;
//   * x and the equilibration scales are read by other lanes through two W-long LDS vectors; the live / bound flags travel as
//     ballot masks, a value of a wave-uniform lane (the pivot, the substitution's current component) through v_readlane;
//   * the equilibrated masked matrix is never stored: A[r][k] = (s_k s_r) P[r][k] for two live rows, the identity's otherwise,
//     recomputed with that association wherever it is used (?potrf's column, ?porfs' residual);
//   * LDS a problem: (2 W S + 2 W) sizeof(T) -- a wave takes 67584 B at W = 64 in double (dynamic LDS, the limit raised by the
//     host: two waves a compute unit), 33792 B at W = 64 in float, 34816 B for its two problems at W = 32 in double (four waves
//     a compute unit each) and 17408 B at W = 32 in float (nine);
//   * no register array, no scratch memory, no global scratch, no barrier: one workgroup is one wave, the lanes of a wave
//     exchange data through LDS behind wave_lds_fence() (common.h).
//
// The arithmetic is the contract of boxqp_active_set (boxqp_rows.h) and posvx_rows16_t (boxqp_rows16.h) with a run-time n:
// classification by relTolerance / absTolerance (QP:239-263), the `s == n` exit with maxIterations (quirk Q8), the reduced
// system's right-hand side as a Kahan-Babuska-Neumaier sum over the bound variables, j ascending (QP:282-305), the multipliers
// as two partial sums (QP:333-337), re-check and applyBounds (QP:339-349), the default limit 10 n + 100; the reduced system is
// solved at full order by a MASKED ?posvx('E','L') -- bound rows are identity rows; ?poequ / ?laqsy over the live rows with
// LAPACK's scond >= 0.1 and small <= amax <= large rule, ?potrf reporting the 1-based index of the first non-positive pivot,
// ?potrs, ?porfs with ITMAX 5 and the berr rule, safe1 = (order + 1) safmin. ?potrf is left-looking by columns (lane r sums
// F[r][k] F[j][k], k ascending, in a register: one LDS write a column instead of a read-modify-write of the trailing matrix),
// ?potrs runs by columns with the vector distributed. Division and square root are the IEEE ones, contraction is off and every
// multiply-add meant as one rounding is __builtin_elementwise_fma.
//
// Identity rows cost nothing: about 70 % of the variables of a typical problem sit on a bound, so a reduced system has a
// third of the rows live. A row k that is live in NO problem of the wave (a wave-uniform ballot mask) is skipped in ?potrf's
// column loop and inner sum, in both sweeps of ?potrs and in ?porfs' residual. Skipping is exact, not approximate: such a row
// and column of F are the identity's (+0 off the diagonal, 1 on it), its right-hand side and solution component are +0, and
// every term left out is fma(a, +0, v) with a = -0 (a = -1 in the row's own lane): the product is -0 and v comes back as it
// is, whatever it is -- or it adds +0 to a sum of absolute values, which is never -0. So a problem's result does not depend on
// whether its wave partner allowed the skip. The first, unconstrained solve has every row live and runs plain loops, unrolled
// so that the LDS reads of eight terms are in flight together.
//
// Independence: the loops run while ANY problem of the wave is still at work (a wave ballot; a problem's own bits decide for
// it) and a finished problem keeps x, status and count through selects, as in boxqp_active_set; beyond the exact skips above
// nothing else branches on data. What a problem returns therefore depends neither on the problem it shares a wave with, nor
// on its half, nor on what the wave solved before it, nor on the grid.
#pragma once

#include "boxqp_rows.h"

namespace mirlsq {

constexpr size_t kBoxQpWaveMinOrder = 17, kBoxQpWaveMaxOrder = 64;

// P count x n x n (row stride n, the lower triangle is read), q and x count x n, l and u n values (bound_stride 0) or count x n
template <class T> struct BoxQpWaveArgs {
    const T* P;
    const T* q;
    const T* l;
    const T* u;
    T* x;                  // in (kBoxQpUnconstrainedSolution) / out
    int* status;           // count
    int* iterations;       // count or nullptr
    int count, n, bound_stride;
    T relTolerance, absTolerance;
    uint32_t maxIterations, flags;
};

// LDS values of one problem and bytes of one wave (64 / W problems)
template <int W> constexpr int boxqp_wave_values() { return 2 * W * (W + 1) + 2 * W; }
template <int W, class T> constexpr size_t boxqp_wave_lds_bytes() { return (size_t)(64 / W) * boxqp_wave_values<W>() * sizeof(T); }

// One problem of order n <= W in the W lanes of half h. Pm, Fm, xv, sv: this problem's LDS.
template <int W, class T> struct BoxQpWave {
    static_assert(W == 32 || W == 64, "one or two problems a wave");
    static constexpr int S = W + 1;
    T* Pm; T* Fm; T* xv; T* sv;
    int n, r, h;
    bool el;               // r < n
    int row;               // the start of this lane's row; lanes that are no element read row 0 (values nobody uses)
    T d_r;                 // P[r][r]

    // the bits of the wave ballot that belong to this lane's problem
    __device__ __forceinline__ unsigned long long bits(bool pred) const
    {
        const unsigned long long b = __builtin_amdgcn_ballot_w64(pred);
        if constexpr (W == 64) return b;
        else return (b >> (32 * h)) & 0xffffffffull;
    }
    // v of lane i of this lane's problem; i is wave-uniform
    __device__ __forceinline__ T bcast(T v, int i) const
    {
        if constexpr (W == 64) return lane_get(v, i);
        else {
            const T a = lane_get(v, i), b = lane_get(v, 32 + i);
            return h ? b : a;
        }
    }
    __device__ __forceinline__ T hmax(T v) const
    {
#pragma unroll
        for (int o = W / 2; o >= 1; o >>= 1) v = vmax(v, __shfl_xor(v, o, 64));
        return v;
    }
    __device__ __forceinline__ T hmin(T v) const
    {
#pragma unroll
        for (int o = W / 2; o >= 1; o >>= 1) v = vmin(v, __shfl_xor(v, o, 64));
        return v;
    }

    // row r of the lower triangle of problem p's matrix into both triangles of Pm: one coalesced row a step
    __device__ __forceinline__ void load(const T* __restrict__ Pg)
    {
        for (int i = 0; i < n; ++i)
            if (r <= i) {
                const T v = Pg[(size_t)i * n + r];
                Pm[i * S + r] = v;
                Pm[r * S + i] = v;
            }
        wave_lds_fence();
        d_r = el ? Pm[r * S + r] : T(0);
    }

    // the masked ?posvx('E','L') at full order: rows with live_r == false are identity rows, `order` is the number of live
    // rows. Hands back component r of the solution and a problem-uniform info (0, or the failed pivot's 1-based index); a
    // problem whose factorization fails keeps computing on values nobody reads.
    __device__ __forceinline__ int posvx(T rhs_r, bool live_r, int order, T& xs_r) const
    {
#pragma clang fp contract(off)
        const T eps = Lim<T>::eps / 2, safmin = Lim<T>::min_normal;
        const bool live = el && live_r;
        const unsigned long long ball = __builtin_amdgcn_ballot_w64(live);
        unsigned long long lm = ball, any = ball;                    // live rows: of this problem, of any problem of the wave
        if constexpr (W == 32) {
            lm = (ball >> (32 * h)) & 0xffffffffull;
            any = (ball | (ball >> 32)) & 0xffffffffull;
        }
        // A row that is live in no problem of the wave is skipped wherever it would add exact zeros (see the header comment):
        // `any` is wave-uniform, and skipping changes no bit of any problem's result. dense: nothing to skip, plain loops.
        const bool dense = any == (n == 64 ? ~0ull : (1ull << n) - 1ull);
        // ?poequ over the live rows
        const T smin = hmin(live ? d_r : Lim<T>::inf());
        const T amax = hmax(live ? d_r : -Lim<T>::inf());
        const bool pos = smin > 0;
        const T scond = vsqrt(smin) / vsqrt(amax);
        const T s_r = (pos && live) ? T(1) / vsqrt(d_r) : T(1);
        const T small = safmin / Lim<T>::eps, large = T(1) / small;
        const bool rcequ = pos && !(scond >= lit<T>(0.1f, 0.1) && amax >= small && amax <= large);
        sv[r] = s_r;
        wave_lds_fence();
        // ?laqsy, never stored: A[r][k]; identity rows / columns for what is not live
        auto A = [&](int k, T sk) {
            const bool lk = ((lm >> k) & 1ull) != 0;
            const T p = Pm[row + k];
            return (live && lk) ? (rcequ ? sk * s_r * p : p) : (r == k ? T(1) : T(0));
        };
        const T b_r = live ? (rcequ ? s_r * rhs_r : rhs_r) : T(0);
        // ?potrf 'L', left-looking by columns
        int info = 0;
        T fd_r = T(1);                                               // F[r][r]
        for (int j = 0; j < n; ++j) {
            if (((any >> j) & 1ull) == 0) {                          // the identity's column
                if (el) Fm[r * S + j] = (r == j) ? T(1) : T(0);
                wave_lds_fence();
                continue;
            }
            T v = A(j, sv[j]);
            const T* Fj = Fm + j * S;
            if (dense) {
#pragma unroll 8
                for (int k = 0; k < j; ++k) v = __builtin_elementwise_fma(-Fm[row + k], Fj[k], v);
            } else {
                for (unsigned long long m = any & ((1ull << j) - 1ull); m; m &= m - 1ull) {
                    const int k = __builtin_ctzll(m);
                    v = __builtin_elementwise_fma(-Fm[row + k], Fj[k], v);
                }
            }
            T ajj = bcast(v, j);
            info = (info == 0 && !(ajj > 0)) ? j + 1 : info;
            ajj = vsqrt(ajj);
            fd_r = (r == j) ? ajj : fd_r;
            if (el) Fm[r * S + j] = (r == j) ? ajj : (r > j ? v / ajj : T(0));
            wave_lds_fence();
        }
        // ?potrs with the vector distributed: L y = v by columns, then L^T z = y by columns of L^T (rows of L)
        const int rc = el ? r : 0;
        auto potrs = [&](T v) {
            for (unsigned long long m = any; m; m &= m - 1ull) {
                const int i = __builtin_ctzll(m);
                const T yi = bcast(v / fd_r, i);
                v = (r == i) ? yi : (r > i ? __builtin_elementwise_fma(-Fm[row + i], yi, v) : v);
            }
            for (unsigned long long m = any; m;) {
                const int i = 63 - __builtin_clzll(m);
                m &= ~(1ull << i);
                const T zi = bcast(v / fd_r, i);
                v = (r == i) ? zi : (r < i ? __builtin_elementwise_fma(-Fm[i * S + rc], zi, v) : v);
            }
            return v;
        };
        T x = potrs(b_r);
        // ?porfs: the loop runs while any problem of the wave refines; a problem that has stopped keeps its solution
        const T safe1 = (T)(order + 1) * safmin, safe2 = safe1 / eps;
        T lstres = 3;
        bool active = true;
        for (int count = 1;; ++count) {
            xv[r] = x;
            wave_lds_fence();
            T ri = b_r, wi = vabs(b_r);
            auto term = [&](int k) {
                const T a = A(k, sv[k]), xk = xv[k];
                ri = __builtin_elementwise_fma(-a, xk, ri);
                wi = __builtin_elementwise_fma(vabs(a), vabs(xk), wi);
            };
            if (dense) {
#pragma unroll 8
                for (int k = 0; k < n; ++k) term(k);
            } else {
                for (unsigned long long m = any; m; m &= m - 1ull) term(__builtin_ctzll(m));
            }
            wave_lds_fence();
            const bool big = wi > safe2;
            const T q = (big ? vabs(ri) : vabs(ri) + safe1) / (big ? wi : wi + safe1);
            const T berr = hmax(live ? q : T(0));
            active = active && berr > eps && 2 * berr <= lstres && count <= 5;
            if (__builtin_amdgcn_ballot_w64(active) == 0) break;
            const T c = potrs(live ? ri : T(0));
            x = active ? x + c : x;
            lstres = active ? berr : lstres;
        }
        xs_r = rcequ ? s_r * x : x;
        return info;
    }

    // boxqp_active_set of boxqp_rows.h with a run-time n. q_r, l_r, u_r: component r (r >= n: ignored). x_r: in, the
    // unconstrained solution when have_x (wave-uniform); out, component r of the solution. status (BoxQPStatus) and iters are
    // problem-uniform.
    __device__ __forceinline__ void active_set(T q_r, T l_r, T u_r, T relTol, T absTol, uint32_t maxIterations, bool have_x, T& x_r,
                                               int& status, int& iters) const
    {
#pragma clang fp contract(off)
        const T lo = el ? l_r : -Lim<T>::inf(), up = el ? u_r : Lim<T>::inf();
        T x = el ? x_r : T(0);
        int st = 0;
        if (!have_x) {                                                       // QP:168-214
            T xs;
            const int info = posvx(-q_r, true, n, xs);
            x = el ? xs : T(0);
            st = info != 0 ? 1 : 0;
        }
        // QP:216-219: a feasible unconstrained solution is the answer (a NaN counts as infeasible)
        const bool infeasible = bits(el && !(lo <= x && x <= up)) != 0;
        bool run = st == 0 && infeasible;
        st = run ? 2 : st;                                                   // QP:378 unless the loop says otherwise
        int it = 0;
        const uint32_t maxit = maxIterations ? maxIterations : (uint32_t)n * 10 + 100;   // QP:224-226
        T la = 0, mu = 0;                                                    // QP:228-232
        int fl = el ? 0 : 2;                                                 // -1 lower, 0 free, 1 upper; 2 = not an element
        for (uint32_t step = 0; step < maxit; ++step) {                      // QP:234
            if (__builtin_amdgcn_ballot_w64(run) == 0) break;
            it = run ? (int)step + 1 : it;
            {                                                                // QP:239-263
                const T xl = x - lo, ux = up - x;
                const bool toL = xl < 0 || (xl < relTol + absTol * vabs(lo) && la >= 0);
                const bool toU = !toL && (ux < 0 || (ux < relTol + absTol * vabs(up) && mu >= 0));
                const bool upd = run && el;
                fl = upd ? (toL ? -1 : (toU ? 1 : 0)) : fl;
                x = upd ? (toL ? lo : (toU ? up : x)) : x;
                la = upd ? (toL ? la : T(0)) : la;
                mu = upd ? (toU ? mu : T(0)) : mu;
            }
            const int sN = __builtin_popcountll(bits(fl == 0));
            run = run && sN != n;                                            // QP:265-266 (quirk Q8): leaves with maxIterations
            // right-hand side of the reduced system, QP:282-305: Kahan-Babuska-Neumaier over the bound variables, j ascending
            const unsigned long long bm = bits(fl == -1 || fl == 1);
            xv[r] = x;                                                       // a bound variable sits ON its bound
            wave_lds_fence();
            T ks = q_r, kc = 0;
#pragma unroll 4
            for (int j = 0; j < n; ++j) {
                const bool bj = ((bm >> j) & 1ull) != 0;
                const T v = Pm[row + j] * xv[j];
                const T t = ks + v;
                const T kn = (vabs(ks) >= vabs(v)) ? kc + ((ks - t) + v) : kc + ((v - t) + ks);
                kc = bj ? kn : kc;
                ks = bj ? t : ks;
            }
            wave_lds_fence();
            const T b_r = -(ks + kc);
            const bool need = run && sN != 0;                                // QP:307-329
            if (__builtin_amdgcn_ballot_w64(need) != 0) {
                T xs;
                const int info = posvx(b_r, fl == 0, sN, xs);
                const bool failed = need && info != 0;
                st = failed ? 1 : st;
                run = run && !failed;
                x = (need && !failed && fl == 0) ? xs : x;
            }
            // multipliers of the bound variables, QP:333-337 (two partial sums, as the reference's two dot products)
            xv[r] = x;
            wave_lds_fence();
            T v1 = 0, v2 = 0;
#pragma unroll 8
            for (int j = 0; j < n; ++j) {
                const T pj = Pm[row + j], xj = xv[j];
                v1 = (j < r) ? __builtin_elementwise_fma(pj, xj, v1) : v1;
                v2 = (j >= r) ? __builtin_elementwise_fma(pj, xj, v2) : v2;
            }
            wave_lds_fence();
            const T val = v1 + v2 + q_r;
            la = (run && fl == -1) ? val : la;
            mu = (run && fl == 1) ? -val : mu;
            // QP:339-347
            const bool again_r = fl == -1 ? !(la >= 0) : (fl == 1 ? !(mu >= 0) : (fl == 0 ? !(x >= lo && x <= up) : false));
            const bool again = bits(again_r) != 0;
            const bool done = run && !again;
            x = (done && el) ? vmax(vmin(x, up), lo) : x;                    // QP:349 applyBounds
            st = done ? 0 : st;
            run = run && again;
        }
        x_r = el ? x : T(0);
        status = st;
        iters = it;
    }
};

// A grid-stride over waves of 64 / W problems; a short last wave at W = 32 repeats the last problem and writes nothing for the
// repeat. Dynamic LDS: boxqp_wave_lds_bytes<W, T>().
template <int W, class T>
__global__ __launch_bounds__(64) void k_boxqp_wave(BoxQpWaveArgs<T> a)
{
    extern __shared__ __align__(16) unsigned char boxqp_wave_lds[];
    constexpr int S = W + 1, PW = 64 / W;
    const int lane = threadIdx.x;
    BoxQpWave<W, T> w;
    w.n = a.n; w.r = lane & (W - 1); w.h = lane / W;
    w.el = w.r < a.n;
    w.row = (w.el ? w.r : 0) * S;
    w.Pm = reinterpret_cast<T*>(boxqp_wave_lds) + w.h * boxqp_wave_values<W>();
    w.Fm = w.Pm + W * S; w.xv = w.Fm + W * S; w.sv = w.xv + W;
    const bool have_x = (a.flags & kBoxQpUnconstrainedSolution) != 0;
    const size_t n = (size_t)a.n;
    for (int p0 = PW * blockIdx.x; p0 < a.count; p0 += PW * gridDim.x) {
        const int p = p0 + w.h < a.count ? p0 + w.h : a.count - 1;
        const size_t pb = (size_t)p * n, bb = (size_t)p * a.bound_stride;
        w.load(a.P + pb * n);
        const T q_r = w.el ? a.q[pb + w.r] : T(0);
        const T l_r = w.el ? a.l[bb + w.r] : T(0), u_r = w.el ? a.u[bb + w.r] : T(0);
        T x_r = (have_x && w.el) ? a.x[pb + w.r] : T(0);
        int st, it;
        w.active_set(q_r, l_r, u_r, a.relTolerance, a.absTolerance, a.maxIterations, have_x, x_r, st, it);
        if (p0 + w.h < a.count) {
            if (w.el) a.x[pb + w.r] = x_r;
            if (w.r == 0) {
                a.status[p] = st;
                if (a.iterations) a.iterations[p] = it;
            }
        }
        wave_lds_fence();                                                    // the next problem's load overwrites Pm
    }
}

}  // namespace mirlsq
