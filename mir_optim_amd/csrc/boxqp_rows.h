// boxqp_rows.h -- solveBoxQP (the reference's mir/optim/boxcqp.d:122-379, cited as QP:) for small orders, FOUR PROBLEMS A WAVE,
// one per 16-lane DPP row (group g = lane >> 4). Two layouts share ONE active-set loop, boxqp_active_set<N, W, T>:
//   * W = 8, n = N <= 8 (this header: boxqp_rows, k_boxqp_rows): the layout of posvx_rows (batched_kernel.h). Lane r = lane & 7
//     of a group holds row r of the group's P and component r of every vector (q, l, u, x, the multipliers, the flags); the
//     upper eight lanes of a group repeat the lower eight.
//   * W = 16, n = N = 9 .. 16 (boxqp_rows16.h: boxqp_rows16, k_boxqp_rows16): lane r = lane & 15, every lane a row of its own.
// A layout hands the loop its masked full-order ?posvx as a callable; everything else is the loop's. No LDS, no barrier, no
// register array indexed at run time.
//
// The loop is the one of solve_wave16.h:203-260 restated for groups that hold DIFFERENT problems:
//   * the reduced system of an active-set step is solved in place at full order by the layout's MASKED ?posvx (a bound
//     variable's row and column are the identity's; ?poequ, berr and safe1 see the free rows and their number only);
//   * its right-hand side is a Kahan-Babuska-Neumaier sum over the bound variables, j ascending (QP:282-305), the multipliers
//     are two partial sums (QP:333-337), classification uses relTolerance / absTolerance (QP:239-263), the re-check and
//     applyBounds follow (QP:339-349);
//   * the loop runs while ANY group of the wave is still iterating (a wave ballot; the group's own bits decide for the group).
//     A group that has finished -- solved, failed factorization, all variables free (quirk Q8), out of iterations -- keeps its x,
//     status and iteration count through selects; nothing branches on a group's data, so what a problem returns does not depend
//     on the three problems it shares a wave with (tests/test_gpu_batched_boxqp.py, tests/test_gpu_batched_boxqp16.py: every
//     rotation of a mixed wave, bit for bit).
// Contraction is off and every multiply-add that is meant to be one rounding is __builtin_elementwise_fma, as in posvx_rows.
#pragma once

#include "batched_kernel.h"

namespace mirlsq {

constexpr uint32_t kBoxQpUnconstrainedSolution = 1u;      // MIR_LSQ_BOX_QP_UNCONSTRAINED_SOLUTION

// the bits of the wave ballot that belong to group g (its 16 lanes; at W = 8 lanes 8..15 repeat lanes 0..7)
__device__ __forceinline__ unsigned rows_bits(bool pred, int g)
{
    return (unsigned)((__builtin_amdgcn_ballot_w64(pred) >> (16 * g)) & 0xffffull);
}

// The active-set loop of both layouts. W: the row width (8 or 16), r = lane & (W - 1). Prow: the full symmetric row r of the
// group's P; q_r, l_r, u_r: component r (r >= N: ignored). solve(rhs_r, live_r, order, T& xs_r) -> info: the layout's masked
// ?posvx of the group's P at full order (rows with live_r == false are identity rows, `order` is the number of live rows); it
// hands back this lane's component of the solution and a group-uniform info (0, or the failed pivot's 1-based index).
// x_r: in, the group's unconstrained solution when have_x (wave-uniform: the reference's unconstrainedSolution = true,
// QP:129, 168, the first solve is then skipped); out, component r of the solution (r >= N: 0). status (BoxQPStatus: 0 solved,
// 1 numericError, 2 maxIterations) and iters (active-set steps, 0 when the unconstrained solution is feasible) are
// group-uniform.
template <int N, int W, class T, class Solve>
__device__ inline void boxqp_active_set(const T (&Prow)[W], T q_r, T l_r, T u_r, T relTol, T absTol, uint32_t maxIterations,
                                                 bool have_x, int r, int g, Solve&& solve, T& x_r, int& status, int& iters)
{
#pragma clang fp contract(off)
    static_assert((W == 8 || W == 16) && N >= 1 && N <= W, "row r = lane & (W - 1)");
    const bool el = r < N;
    const T lo = el ? l_r : -Lim<T>::inf(), up = el ? u_r : Lim<T>::inf();
    T x = el ? x_r : T(0);
    int st = 0;
    if (!have_x) {                                                       // QP:168-214
        T xs;
        const int info = solve(-q_r, true, N, xs);
        x = el ? xs : T(0);
        st = info != 0 ? 1 : 0;
    }
    // QP:216-219: a feasible unconstrained solution is the answer (a NaN counts as infeasible)
    const bool infeasible = rows_bits(el && !(lo <= x && x <= up), g) != 0;
    bool run = st == 0 && infeasible;
    st = run ? 2 : st;                                                   // QP:378 unless the loop says otherwise
    int it = 0;
    const uint32_t maxit = maxIterations ? maxIterations : (uint32_t)N * 10 + 100;   // QP:224-226
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
        const int sN = __builtin_popcount(rows_bits(fl == 0, g) & ((1u << W) - 1u));   // W = 8: lanes 8..15 repeat
        run = run && sN != N;                                            // QP:265-266 (quirk Q8): leaves with maxIterations
        // right-hand side of the reduced system, QP:282-305: Kahan-Babuska-Neumaier over the bound variables, j ascending
        T ks = q_r, kc = 0;
        static_for<W>([&](auto JX) {
            constexpr int j = JX.value;
            if constexpr (j < N) {
                const bool bj = dpp_row_bcast<j>(fl) != 0;
                const T xj = dpp_row_bcast<j>(x);                        // a bound variable sits ON its bound
                const T v = Prow[j] * xj;
                const T t = ks + v;
                const T kn = (vabs(ks) >= vabs(v)) ? kc + ((ks - t) + v) : kc + ((v - t) + ks);
                kc = bj ? kn : kc;
                ks = bj ? t : ks;
            }
        });
        const T b_r = -(ks + kc);
        const bool need = run && sN != 0;                                // QP:307-329
        if (__builtin_amdgcn_ballot_w64(need) != 0) {
            T xs;
            const int info = solve(b_r, fl == 0, sN, xs);
            const bool failed = need && info != 0;
            st = failed ? 1 : st;
            run = run && !failed;
            x = (need && !failed && fl == 0) ? xs : x;
        }
        // multipliers of the bound variables, QP:333-337 (two partial sums, as the reference's two dot products)
        T v1 = 0, v2 = 0;
        static_for<W>([&](auto JX) {
            constexpr int j = JX.value;
            if constexpr (j < N) {
                const T xj = dpp_row_bcast<j>(x);
                v1 = (j < r) ? __builtin_elementwise_fma(Prow[j], xj, v1) : v1;
                v2 = (j >= r) ? __builtin_elementwise_fma(Prow[j], xj, v2) : v2;
            }
        });
        const T val = v1 + v2 + q_r;
        la = (run && fl == -1) ? val : la;
        mu = (run && fl == 1) ? -val : mu;
        // QP:339-347
        const bool again_r = fl == -1 ? !(la >= 0) : (fl == 1 ? !(mu >= 0) : (fl == 0 ? !(x >= lo && x <= up) : false));
        const bool again = rows_bits(again_r, g) != 0;
        const bool done = run && !again;
        x = (done && el) ? vmax(vmin(x, up), lo) : x;                    // QP:349 applyBounds
        st = done ? 0 : st;
        run = run && again;
    }
    x_r = el ? x : T(0);
    status = st;
    iters = it;
}

// n = N <= 8 in the layout of posvx_rows (r = lane & 7); arguments as boxqp_active_set's. The callable is a struct as in
// boxqp_rows16 (boxqp_rows16.h says why).
template <int N, int NMAX, class T>
__device__ inline void boxqp_rows(const T (&Prow)[NMAX], T q_r, T l_r, T u_r, T relTol, T absTol, uint32_t maxIterations,
                                  bool have_x, int r, int g, T& x_r, int& status, int& iters)
{
    static_assert(NMAX == 8, "row r = lane & 7");
    struct {
        const T (&Prow)[NMAX]; int r;
        __device__ __forceinline__ int operator()(T rhs_r, bool live_r, int order, T& xs_r) const
        {
#pragma clang fp contract(off)
            T xs[NMAX];
            const int info = posvx_rows<N, NMAX, T, true>(Prow, rhs_r, r, xs, live_r, order);
            xs_r = MIRLSQ_ROW_PICK(xs, r);
            return info;
        }
    } solve{Prow, r};
    boxqp_active_set<N, NMAX, T>(Prow, q_r, l_r, u_r, relTol, absTol, maxIterations, have_x, r, g, solve, x_r, status, iters);
}

// the arguments of k_boxqp_rows (W = 8) and of k_boxqp_rows16 (W = 16)
template <class T> struct BoxQpRowsArgs {
    const T* P;            // count x W^2, row stride W, lower triangle read
    const T* q;            // count x W
    const T* l;            // W (bound_stride 0) or count x W
    const T* u;
    T* x;                  // count x W, in (kBoxQpUnconstrainedSolution) / out
    int* status;           // count
    int* iterations;       // count or nullptr
    int count, bound_stride;
    T relTolerance, absTolerance;
    uint32_t maxIterations, flags;
};

// a grid-stride over groups of four problems; a short last wave repeats the last problem and writes nothing for the repeats
template <int N, class T>
__global__ __launch_bounds__(64) void k_boxqp_rows(BoxQpRowsArgs<T> a)
{
    const int lane = threadIdx.x, r = lane & 7, g = lane >> 4;
    const bool have_x = (a.flags & kBoxQpUnconstrainedSolution) != 0;
    for (int p0 = 4 * blockIdx.x; p0 < a.count; p0 += 4 * gridDim.x) {
        const int p = p0 + g < a.count ? p0 + g : a.count - 1;
        const size_t pb = (size_t)p * 8, bb = (size_t)p * a.bound_stride;
        T Prow[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) Prow[k] = (r < N && k < N) ? a.P[(size_t)p * 64 + (k <= r ? r * 8 + k : k * 8 + r)] : T(0);
        const T q_r = r < N ? a.q[pb + r] : T(0);
        const T l_r = r < N ? a.l[bb + r] : T(0), u_r = r < N ? a.u[bb + r] : T(0);
        T x_r = (have_x && r < N) ? a.x[pb + r] : T(0);
        int st, it;
        boxqp_rows<N, 8, T>(Prow, q_r, l_r, u_r, a.relTolerance, a.absTolerance, a.maxIterations, have_x, r, g, x_r, st, it);
        if (p0 + g < a.count) {
            if ((lane & 15) < 8) a.x[pb + r] = x_r;                      // components >= N are written as 0
            if ((lane & 15) == 0) {
                a.status[p] = st;
                if (a.iterations) a.iterations[p] = it;
            }
        }
    }
}

}  // namespace mirlsq
