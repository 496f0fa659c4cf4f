// batched_bounded.h -- the bounded step of the batched one-wavefront-per-problem fit: what k_lm_batched (batched_kernel.h) does,
// in an instance compiled with this policy, when the damped step of a ladder level leaves the box. The reference solves
//     min 1/2 d^T (J^T J + lambda I) d + (J^T y)^T d,    lower - x <= d <= upper - x                      (LS:1074-1085)
// with solveBoxQP (boxcqp.d:122-379); here that is boxqp_rows<N, 8, T> (boxqp_rows.h: the active-set loop in the register
// layout of posvx_rows, no LDS, no barrier), called with the level's unconstrained solution, so the first solve is not repeated.
// The four 16-lane groups of the wave hold the SAME system (the loop's ballots are then wave-uniform); the step is read from
// group 0. The default instances of the kernel do not include this header and are not changed by it.
#pragma once

#include "boxqp_rows.h"

namespace mirlsq {

struct BatchedBoxQpStep {
    static constexpr bool enabled = true;
    // JJrow: row r of J^T J (undamped); Jy_r: component r of J^T y; lambda: the damping of the level in use (quirk Q1: added to
    // the diagonal as the kernel's own solve adds it); lo, up, x: replicated; sol: in, the level's unconstrained solution
    // (replicated); out, the step of the box QP (replicated; components >= N are 0). false: the QP did not end as solved (LS:1080).
    template <int N, class T>
    __device__ static inline bool step(const T (&JJrow)[kBatchedNMax], T Jy_r, T lambda, const T (&lo)[kBatchedNMax],
                                       const T (&up)[kBatchedNMax], const T (&x)[kBatchedNMax], const LmSettingsDev<T>& S, int r, int g,
                                       T (&sol)[kBatchedNMax])
    {
#pragma clang fp contract(off)
        constexpr int NMAX = kBatchedNMax;
        T Prow[NMAX], ql[NMAX], qu[NMAX];
#pragma unroll
        for (int k = 0; k < NMAX; ++k) {
            Prow[k] = JJrow[k] + ((k == r && r < N) ? lambda : T(0));   // (Q1), as the ladder forms it
            ql[k] = lo[k] - x[k];                                        // LS:1074-1077
            qu[k] = up[k] - x[k];
        }
        T x_r = MIRLSQ_ROW_PICK(sol, r);
        int status, iters;
        boxqp_rows<N, NMAX, T>(Prow, Jy_r, MIRLSQ_ROW_PICK(ql, r), MIRLSQ_ROW_PICK(qu, r), S.qpRelTolerance, S.qpAbsTolerance,
                               S.qpMaxIterations, true, r, g, x_r, status, iters);
#pragma unroll
        for (int j = 0; j < NMAX; ++j) sol[j] = j < N ? lane_get(x_r, j) : T(0);
        return __builtin_amdgcn_readfirstlane(status) == 0;
    }
};

}  // namespace mirlsq
