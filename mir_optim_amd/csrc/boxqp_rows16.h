// boxqp_rows16.h -- solveBoxQP (the reference's mir/optim/boxcqp.d:122-379, cited as QP:) for n = N = 9 .. 16, FOUR PROBLEMS A WAVE,
// one per 16-lane DPP row (group g = lane >> 4): lane r = lane & 15 of a group holds row r of the group's P and component r of
// EVERY vector (q, l, u, x, the two multiplier vectors, the flag) -- the distributed layout of posvx_rows16 (solve_wave16.h),
// not the one of posvx_rows (batched_kernel.h), whose replicated x[NMAX] in every lane would not fit the register file at
// sixteen rows. Rows >= N are identity rows and not elements. No LDS, no barrier, no register array indexed at run time.
//
// The active-set loop is boxqp_active_set of boxqp_rows.h, the one loop of both layouts; this header gives it the masked solve
// at full order by the 16-row ?posvx: for double posvx_rows16 of solve_wave16.h as it is, for float the restatement below
// (IEEE division and square root as in posvx_rows). What the loop promises holds here as there: what a problem returns does
// not depend on its three wave partners (tests/test_gpu_batched_boxqp16.py: every rotation of a mixed wave, bit for bit).
// Contraction is off and every multiply-add that is meant to be one rounding is __builtin_elementwise_fma / fma.
#pragma once

#include "boxqp_rows.h"
#include "solve_wave16.h"

namespace mirlsq {

template <class T> __device__ __forceinline__ T row16_vmax(T v)
{
    v = vmax(v, dpp_row_ror<8>(v)); v = vmax(v, dpp_row_ror<4>(v)); v = vmax(v, dpp_row_ror<2>(v)); v = vmax(v, dpp_row_ror<1>(v));
    return v;
}
template <class T> __device__ __forceinline__ T row16_vmin(T v)
{
    v = vmin(v, dpp_row_ror<8>(v)); v = vmin(v, dpp_row_ror<4>(v)); v = vmin(v, dpp_row_ror<2>(v)); v = vmin(v, dpp_row_ror<1>(v));
    return v;
}

// ?posvx('E','L') of the group's system M x = rhs in the layout of posvx_rows16, for any value type: Mrow = row r of the
// symmetric M, d_r = Mrow[r] (handed in: picking it out of the register array with a run-time index would put the array in
// scratch memory); rows with live == false (and every row >= N) are identity rows, `order` is the number of live rows.
// ?poequ / ?laqsy over the live rows, right-looking ?potrf, ?potrs with the vector distributed (component r in lane r), ?porfs
// with ITMAX 5 and LAPACK's berr rule, where a group that stopped refining keeps its solution. Division and square root are
// the IEEE ones, as in posvx_rows. Returns info (group-uniform: 0, or the 1-based index of the first non-positive pivot); a
// group whose factorization fails keeps computing on values nobody reads.
template <int N, class T>
__device__ __forceinline__ int posvx_rows16_t(const T (&Mrow)[kW16], T d_r, T rhs_r, bool live_r, int r, T& x_r, int order)
{
#pragma clang fp contract(off)
    const T eps = Lim<T>::eps / 2, safmin = Lim<T>::min_normal;
    const bool live = r < N && live_r;
    // ?poequ over the live rows
    const T smin = row16_vmin(live ? d_r : Lim<T>::inf());
    const T amax = row16_vmax(live ? d_r : -Lim<T>::inf());
    const bool pos = smin > 0;
    const T scond = vsqrt(smin) / vsqrt(amax);
    const T s_r = (pos && live) ? T(1) / vsqrt(d_r) : T(1);
    const T small = safmin / Lim<T>::eps, large = T(1) / small;
    const bool rcequ = pos && !(scond >= lit<T>(0.1f, 0.1) && amax >= small && amax <= large);
    // ?laqsy; identity rows / columns for what is not live
    T Arow[kW16], Frow[kW16], Fcol[kW16];                        // Fcol[k] = F[k][r], k > r: column r of the factor, for L^T
    static_for<kW16>([&](auto K) {
        constexpr int k = K.value;
        const T sk = dpp_row_bcast<k>(s_r);
        const bool lk = dpp_row_bcast<k>(live ? 1 : 0) != 0;
        Arow[k] = (live && lk && k < N) ? (rcequ ? sk * s_r * Mrow[k] : Mrow[k]) : (r == k ? T(1) : T(0));
        Frow[k] = Arow[k];
        Fcol[k] = T(0);
    });
    const T b_r = live ? (rcequ ? s_r * rhs_r : rhs_r) : T(0);
    // ?potrf 'L', right-looking by columns: after step j, Frow[jj] (jj > j) of row r >= jj holds A[r][jj] - sum_{k <= j} F[r][k] F[jj][k]
    int info = 0;
    T fd_r = T(1);                                               // F[r][r]
    static_for<kW16>([&](auto J) {
        constexpr int j = J.value;
        if constexpr (j < N) {
            T ajj = dpp_row_bcast<j>(Frow[j]);
            info = (info == 0 && !(ajj > 0)) ? j + 1 : info;
            ajj = vsqrt(ajj);
            const T q = Frow[j] / ajj;
            Frow[j] = (r == j) ? ajj : q;                        // rows above the diagonal carry values nobody reads
            fd_r = (r == j) ? ajj : fd_r;
            static_for<kW16>([&](auto JJ) {
                constexpr int jj = JJ.value;
                if constexpr (jj > j && jj < N) {
                    const T ljj = dpp_row_bcast<jj>(Frow[j]);    // F[jj][j]
                    Frow[jj] = __builtin_elementwise_fma(-Frow[j], ljj, Frow[jj]);
                    Fcol[jj] = (r == j) ? ljj : Fcol[jj];        // lane j collects column j of the factor
                }
            });
        }
    });
    // ?potrs with the vector distributed: L y = v by columns, then L^T z = y by columns of L^T
    auto potrs = [&](T v) {
        static_for<kW16>([&](auto I) {
            constexpr int i = I.value;
            if constexpr (i < N) {
                const T yi = dpp_row_bcast<i>(v / fd_r);
                v = (r == i) ? yi : (r > i ? __builtin_elementwise_fma(-Frow[i], yi, v) : v);
            }
        });
        static_for<kW16>([&](auto II) {
            constexpr int i = kW16 - 1 - II.value;
            if constexpr (i < N) {
                const T zi = dpp_row_bcast<i>(v / fd_r);
                v = (r == i) ? zi : (r < i ? __builtin_elementwise_fma(-Fcol[i], zi, v) : v);
            }
        });
        return v;
    };
    T x = potrs(b_r);
    // ?porfs: the loop runs while any group refines; a group that has stopped keeps its solution
    const T safe1 = (T)(order + 1) * safmin, safe2 = safe1 / eps;
    T lstres = 3;
    bool active = true;
    for (int count = 1;; ++count) {
        T ri = b_r, wi = vabs(b_r);
        static_for<kW16>([&](auto K) {
            constexpr int k = K.value;
            if constexpr (k < N) {
                const T xk = dpp_row_bcast<k>(x);
                ri = __builtin_elementwise_fma(-Arow[k], xk, ri);
                wi = __builtin_elementwise_fma(vabs(Arow[k]), vabs(xk), wi);
            }
        });
        const bool big = wi > safe2;
        const T q = (big ? vabs(ri) : vabs(ri) + safe1) / (big ? wi : wi + safe1);
        const T berr = row16_vmax(live ? q : T(0));
        active = active && berr > eps && 2 * berr <= lstres && count <= 5;
        if (__builtin_amdgcn_ballot_w64(active) == 0) break;
        const T c = potrs(live ? ri : T(0));
        x = active ? x + c : x;
        lstres = active ? berr : lstres;
    }
    x_r = rcequ ? s_r * x : x;
    return info;
}

// the 16-row ?posvx of value type T: double goes through posvx_rows16 of solve_wave16.h as it is (no shift), float through
// the restatement above
template <int N, class T>
__device__ __forceinline__ int posvx16(const T (&Mrow)[kW16], T d_r, T rhs_r, bool live, int r, T& x_r, int order)
{
    if constexpr (std::is_same<T, double>::value) return posvx_rows16<N>(Mrow, 0.0, d_r, rhs_r, r < N && live, r, x_r, order);
    else return posvx_rows16_t<N, T>(Mrow, d_r, rhs_r, live, r, x_r, order);
}

// n = N = 9 .. 16 (r = lane & 15): boxqp_active_set of boxqp_rows.h with the 16-row ?posvx. d_r = Prow[r]; the other arguments
// as boxqp_active_set's. The callable is a struct, not a lambda: with a lambda the compiler orders a few instructions of the
// N = 15 and 16 instances differently; with the struct all sixteen compile to the code of the loop written out here.
template <int N, class T>
__device__ inline void boxqp_rows16(const T (&Prow)[kW16], T d_r, T q_r, T l_r, T u_r, T relTol, T absTol, uint32_t maxIterations,
                                    bool have_x, int r, int g, T& x_r, int& status, int& iters)
{
    static_assert(N >= 9, "n <= 8 is boxqp_rows");
    struct {
        const T (&Prow)[kW16]; T d_r; int r;
        __device__ __forceinline__ int operator()(T rhs_r, bool live_r, int order, T& xs_r) const
        {
#pragma clang fp contract(off)
            return posvx16<N, T>(Prow, d_r, rhs_r, live_r, r, xs_r, order);
        }
    } solve{Prow, d_r, r};
    boxqp_active_set<N, kW16, T>(Prow, q_r, l_r, u_r, relTol, absTol, maxIterations, have_x, r, g, solve, x_r, status, iters);
}

// row r of problem p's symmetric matrix from its lower triangle (rows and columns >= N: 0), and its diagonal entry
template <int N, class T>
__device__ __forceinline__ void load_row16(const T* __restrict__ P, int p, int r, T (&Prow)[kW16], T& d_r)
{
    const T* Pp = P + (size_t)p * (kW16 * kW16);
#pragma unroll
    for (int k = 0; k < kW16; ++k) Prow[k] = (r < N && k < N) ? Pp[k <= r ? r * kW16 + k : k * kW16 + r] : T(0);
    d_r = r < N ? Pp[r * kW16 + r] : T(0);
}

// a grid-stride over groups of four problems; a short last wave repeats the last problem and writes nothing for the repeats
template <int N, class T>
__global__ __launch_bounds__(64) void k_boxqp_rows16(BoxQpRowsArgs<T> a)
{
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const bool have_x = (a.flags & kBoxQpUnconstrainedSolution) != 0;
    for (int p0 = 4 * blockIdx.x; p0 < a.count; p0 += 4 * gridDim.x) {
        const int p = p0 + g < a.count ? p0 + g : a.count - 1;
        const size_t pb = (size_t)p * kW16, bb = (size_t)p * a.bound_stride;
        T Prow[kW16], d_r;
        load_row16<N, T>(a.P, p, r, Prow, d_r);
        const T q_r = r < N ? a.q[pb + r] : T(0);
        const T l_r = r < N ? a.l[bb + r] : T(0), u_r = r < N ? a.u[bb + r] : T(0);
        T x_r = (have_x && r < N) ? a.x[pb + r] : T(0);
        int st, it;
        boxqp_rows16<N, T>(Prow, d_r, q_r, l_r, u_r, a.relTolerance, a.absTolerance, a.maxIterations, have_x, r, g, x_r, st, it);
        if (p0 + g < a.count) {
            a.x[pb + r] = x_r;                                           // components >= N are written as 0
            if (r == 0) {
                a.status[p] = st;
                if (a.iterations) a.iterations[p] = it;
            }
        }
    }
}

// unit-test entry of the unmasked 16-row ?posvx: four systems a wave; P count x 256 (row-major, lower triangle read), rhs and
// x count x 16; x of a system whose factorization failed is written as 0
template <int N, class T>
__global__ __launch_bounds__(64) void k_posvx_rows16(const T* __restrict__ P, const T* __restrict__ rhs, int count,
                                                     T* __restrict__ x, int* __restrict__ info)
{
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    for (int p0 = 4 * blockIdx.x; p0 < count; p0 += 4 * gridDim.x) {
        const int p = p0 + g < count ? p0 + g : count - 1;              // a short last wave repeats the last system
        T Prow[kW16], d_r, sol;
        load_row16<N, T>(P, p, r, Prow, d_r);
        const int rc = posvx16<N, T>(Prow, d_r, r < N ? rhs[(size_t)p * kW16 + r] : T(0), true, r, sol, N);
        if (p0 + g < count) {
            x[(size_t)p * kW16 + r] = (rc == 0 && r < N) ? sol : T(0);
            if (r == 0) info[p] = rc;
        }
    }
}

}  // namespace mirlsq
