// spd_inverse.h -- X = inv(P) of a symmetric positive definite n x n matrix on the device, any n: what turns the J^T J of a
// fresh Jacobian refresh into the covariance of the fitted parameters (Solver<T>::covariance, covariance.hip).
//
//   k_spd_factor   ONE workgroup. Equilibrates as ?posvx('E') does (?poequ / ?laqsy: s_j = 1 / sqrt(P_jj), applied when
//                  posvx_rows of batched_kernel.h applies it), then factors A = S P S = L L^T by a right-looking lower Cholesky in
//                  16-column panels: the 16 x 16 diagonal block in LDS (one wave), the rows below it one row per thread, the
//                  trailing matrix in 4 x 4 register tiles. The matrix lives in the n x n scratch W in global memory (L2
//                  resident up to n ~ 1024): L in the lower triangle and, mirrored, L^T in the upper one, so that every
//                  later access runs ALONG a row of W.
//   k_spd_columns  n workgroups of one wave. Wave c solves L z = e_c and L^T v = z for the rows >= c only (column c of the
//                  inverse below its diagonal; the work is ~ (n - c)^2) and writes X[i][c] = X[c][i] = s_i s_c v_i: the same
//                  value to both places, X is symmetric to the bit.
// The two phases are two launches on the caller's stream; no workgroup waits for another one. Every sum runs in a fixed order
// (k ascending), every multiply-add is an explicit fma with contraction off, there are no atomics: same input, same bits.
//
// fixed (n bytes or nullptr): a fixed index is taken out of the system -- its row and column are those of the identity while
// factoring (entries of P there are never read) and 0 in X. info: 0, or the 1-based order among the FREE indices of the first
// leading minor that is not positive (a NaN takes the same exit: !(a_jj > 0)); then every free entry of X is +inf.
#pragma once

#include "common.h"

namespace mirlsq {

constexpr int kInvPanel = 16;         // panel width of the factorization
constexpr int kInvThreads = 1024;     // k_spd_factor's workgroup

template <typename T>
__device__ inline bool inv_fixed(const unsigned char* fixed, int i) { return fixed != nullptr && fixed[i] != 0; }

template <typename T>
__global__ __launch_bounds__(kInvThreads) void k_spd_factor(int n, const T* __restrict__ P, const unsigned char* __restrict__ fixed,
                                                            T* __restrict__ W, T* __restrict__ s, int* __restrict__ info)
{
#pragma clang fp contract(off)
    constexpr int NB = kInvPanel, NW = kInvThreads / kWave;
    __shared__ T D[NB][NB + 1];
    __shared__ T red_mn[NW], red_mx[NW];
    __shared__ int s_rcequ, s_fail;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t ld = (size_t)n;

    // ---- ?poequ over the free indices: smallest and largest diagonal entry (a NaN is ignored here, as fmin / fmax do in
    //      posvx_rows; it fails the factorization at its own index)
    T mn = Lim<T>::inf(), mx = -Lim<T>::inf();
    for (int j = tid; j < n; j += kInvThreads) {
        if (inv_fixed<T>(fixed, j)) continue;
        const T d = P[(size_t)j * ld + j];
        mn = dfmin(mn, d);
        mx = dfmax(mx, d);
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    if (lane == 0) { red_mn[wave] = mn; red_mx[wave] = mx; }
    if (tid == 0) s_fail = 0;
    __syncthreads();
    if (tid == 0) {
        T smin = red_mn[0], amax = red_mx[0];
        for (int w = 1; w < NW; ++w) { smin = dfmin(smin, red_mn[w]); amax = dfmax(amax, red_mx[w]); }
        const bool pos = smin > 0;
        const T scond = dsqrt(smin) / dsqrt(amax);
        const T small = Lim<T>::min_normal / Lim<T>::eps, large = T(1) / small;
        s_rcequ = (pos && !(scond >= T(0.1) && amax >= small && amax <= large)) ? 1 : 0;
    }
    __syncthreads();
    const bool rcequ = s_rcequ != 0;
    for (int j = tid; j < n; j += kInvThreads)
        s[j] = (rcequ && !inv_fixed<T>(fixed, j)) ? T(1) / dsqrt(P[(size_t)j * ld + j]) : T(1);
    __syncthreads();

    // ---- ?laqsy: the lower triangle of S P S into W; a fixed index gets the identity's row and column
    for (int i = wave; i < n; i += NW) {
        const bool fi = inv_fixed<T>(fixed, i);
        const T si = s[i];
        for (int j = lane; j <= i; j += kWave) {
            T v;
            if (fi || inv_fixed<T>(fixed, j)) v = (i == j) ? T(1) : T(0);
            else {
                v = P[(size_t)i * ld + j];
                if (rcequ) v = (s[j] * si) * v;
            }
            W[(size_t)i * ld + j] = v;
        }
    }
    __syncthreads();

    for (int k0 = 0; k0 < n; k0 += NB) {
        const int w = (n - k0) < NB ? (n - k0) : NB;
        const int k1 = k0 + w;
        // ---- the diagonal block: ?potf2 'L' by wave 0 in LDS
        if (tid < NB * NB) {
            const int r = tid / NB, c = tid % NB;
            if (r < w && c <= r) D[r][c] = W[(size_t)(k0 + r) * ld + k0 + c];
        }
        __syncthreads();
        if (wave == 0) {
            const int r = lane & 15, cg = lane >> 4;
            for (int j = 0; j < w; ++j) {
                const T ajj = D[j][j];
                if (!(ajj > 0)) {                          // wave-uniform: not positive definite (or a NaN)
                    if (lane == 0) s_fail = k0 + j + 1;
                    break;
                }
                const T d = dsqrt(ajj);
                wave_lds_fence();
                if (cg == 0 && r > j && r < w) D[r][j] = D[r][j] / d;
                if (lane == 0) D[j][j] = d;
                wave_lds_fence();
                for (int c = j + 1 + cg; c < w; c += 4)
                    if (r >= c && r < w) D[r][c] = dfma(-D[r][j], D[c][j], D[r][c]);
                wave_lds_fence();
            }
        }
        __syncthreads();
        if (s_fail) break;
        // ---- the factored block back to W, lower and mirrored
        if (tid < NB * NB) {
            const int r = tid / NB, c = tid % NB;
            if (r < w && c <= r) {
                const T v = D[r][c];
                W[(size_t)(k0 + r) * ld + k0 + c] = v;
                W[(size_t)(k0 + c) * ld + k0 + r] = v;
            }
        }
        // ---- the rows below: L[i][k0..k1) = A[i][k0..k1) inv(L_kk^T), one row per thread
        for (int i = k1 + tid; i < n; i += kInvThreads) {
            asm volatile("" ::: "memory");       // D is re-read per row: hoisted out of the loop its 136 values take the register file
            T* row = W + (size_t)i * ld + k0;
            T x[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) x[j] = j < w ? row[j] : T(0);
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (j < w) {
                    T t = x[j];
#pragma unroll
                    for (int k = 0; k < j; ++k) t = dfma(-x[k], D[j][k], t);
                    x[j] = t / D[j][j];
                }
            }
#pragma unroll
            for (int j = 0; j < NB; ++j)
                if (j < w) {
                    row[j] = x[j];
                    W[(size_t)(k0 + j) * ld + i] = x[j];
                }
        }
        __syncthreads();
        // ---- the trailing matrix: A[i][j] -= sum_k L[i][k] L[j][k], i >= j >= k1, in 4 x 4 tiles a thread; the panel is read
        //      from its mirror (rows k0..k1 of W: consecutive threads read consecutive addresses)
        const int nr = n - k1;
        if (nr > 0) {
            const int nt = (nr + 3) / 4;
            const int tiles = nt * (nt + 1) / 2;
            for (int t = tid; t < tiles; t += kInvThreads) {
                // t -> (bi, bj) of the lower triangle of tiles; the float estimate is corrected by the two loops, so the decode is exact
                // for every t an int holds (tiles < 2^24 up to n = 23 000)
                int bi = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
                while (bi * (bi + 1) / 2 > t) --bi;
                while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
                const int bj = t - bi * (bi + 1) / 2;
                const int i0 = k1 + 4 * bi, j0 = k1 + 4 * bj;
                int ii[4], jj[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    ii[q] = (i0 + q < n) ? i0 + q : n - 1;     // clamped for the loads; the stores are guarded
                    jj[q] = (j0 + q < n) ? j0 + q : n - 1;
                }
                T c[4][4];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)      // (above the diagonal nothing has been written and nothing is stored: not read)
                        c[a][b] = (i0 + a < n && j0 + b <= i0 + a) ? W[(size_t)(i0 + a) * ld + j0 + b] : T(0);
                for (int k = 0; k < w; ++k) {
                    const T* prow = W + (size_t)(k0 + k) * ld;
                    T av[4], bv[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) { av[q] = prow[ii[q]]; bv[q] = prow[jj[q]]; }
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) c[a][b] = dfma(-av[a], bv[b], c[a][b]);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (i0 + a < n && j0 + b <= i0 + a) W[(size_t)(i0 + a) * ld + j0 + b] = c[a][b];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        int rank = 0;
        if (s_fail) for (int j = 0; j < s_fail; ++j) rank += inv_fixed<T>(fixed, j) ? 0 : 1;
        *info = rank;
    }
}

// column c of the inverse from the diagonal down, by one wave; dynamic LDS: n - c elements (the vector z, then v in place)
template <typename T>
__global__ __launch_bounds__(kWave) void k_spd_columns(int n, const T* __restrict__ W, const T* __restrict__ s,
                                                       const unsigned char* __restrict__ fixed, const int* __restrict__ info,
                                                       T* __restrict__ X)
{
#pragma clang fp contract(off)
    extern __shared__ double spd_columns_lds[];
    T* z = reinterpret_cast<T*>(spd_columns_lds);
    const int c = blockIdx.x, lane = threadIdx.x, nn = n - c;
    const size_t ld = (size_t)n;
    const bool fc = inv_fixed<T>(fixed, c);
    if (fc || *info != 0) {
        for (int r = lane; r < nn; r += kWave) {
            const int i = c + r;
            const T v = (fc || inv_fixed<T>(fixed, i)) ? T(0) : Lim<T>::inf();
            X[(size_t)i * ld + c] = v;
            X[(size_t)c * ld + i] = v;
        }
        return;
    }
    const int nblk = (nn + kWave - 1) / kWave;
    // ---- L z = e_c, 64 rows at a time: the earlier blocks' z from LDS, then the block's own triangle lane by lane.
    //      L[i][k] is read as W[c + k][i] (the mirror): one row of W per k, consecutive lanes consecutive addresses
    for (int b = 0; b < nblk; ++b) {
        const int r0 = b * kWave, r = r0 + lane;
        const int i = c + (r < nn ? r : nn - 1);
        T t = r == 0 ? T(1) : T(0);
#pragma unroll 8
        for (int k = 0; k < r0; ++k) t = dfma(-W[(size_t)(c + k) * ld + i], z[k], t);
        const T dinv = T(1) / W[(size_t)i * ld + i];
        const int cnt = (nn - r0) < kWave ? (nn - r0) : kWave;
        for (int j = 0; j < cnt; ++j) {
            const T zj = lane_bcast(t * dinv, j);
            const T lj = W[(size_t)(c + r0 + j) * ld + i];
            if (lane > j) t = dfma(-lj, zj, t);
            if (lane == j) t = zj;
        }
        if (r < nn) z[r] = t;
        __syncthreads();
    }
    // ---- L^T v = z from the last block up: L[k][i], k > i, is W[c + k][i] of the lower triangle
    for (int b = nblk - 1; b >= 0; --b) {
        const int r0 = b * kWave, r = r0 + lane;
        const int i = c + (r < nn ? r : nn - 1);
        T t = r < nn ? z[r] : T(0);
#pragma unroll 8
        for (int k = r0 + kWave; k < nn; ++k) t = dfma(-W[(size_t)(c + k) * ld + i], z[k], t);
        const T dinv = T(1) / W[(size_t)i * ld + i];
        const int cnt = (nn - r0) < kWave ? (nn - r0) : kWave;
        for (int j = cnt - 1; j >= 0; --j) {
            const T vj = lane_bcast(t * dinv, j);
            const T lj = W[(size_t)(c + r0 + j) * ld + i];
            if (lane < j) t = dfma(-lj, vj, t);
            if (lane == j) t = vj;
        }
        __syncthreads();
        if (r < nn) z[r] = t;
        __syncthreads();
    }
    // ---- undo the scaling, write the column and its mirror
    const T sc = s[c];
    for (int r = lane; r < nn; r += kWave) {
        const int i = c + r;
        const T v = inv_fixed<T>(fixed, i) ? T(0) : (s[i] * sc) * z[r];
        X[(size_t)i * ld + c] = v;
        X[(size_t)c * ld + i] = v;
    }
}

// cov = s^2 X at the free entries, s^2 = sum[0] / (rows - n_free) (1 with `absolute`); no degrees of freedom: +inf. Entries of
// fixed rows / columns (0) and the +inf of a failed inverse are left alone. rows: `rows_host`, or with `rows_dev` the all-reduced
// total sum[1] * 4096 + sum[2] (two limbs, so that a float sum over the ranks stays exact).
template <typename T>
__global__ __launch_bounds__(256) void k_cov_scale(int n, T* __restrict__ X, const unsigned char* __restrict__ fixed,
                                                   const int* __restrict__ info, const T* __restrict__ sum, int rows_dev,
                                                   double rows_host, double n_free, int absolute)
{
#pragma clang fp contract(off)
    if (*info != 0) return;
    const double rows = rows_dev ? (double)sum[1] * 4096.0 + (double)sum[2] : rows_host;
    const double dof = rows - n_free;
    const bool none = !absolute && !(dof > 0);
    if (absolute && !none) return;
    const T s2 = none ? Lim<T>::inf() : sum[0] / (T)dof;
    const size_t total = (size_t)n * n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx / n), j = (int)(idx % n);
        if (inv_fixed<T>(fixed, i) || inv_fixed<T>(fixed, j)) continue;
        X[idx] = none ? Lim<T>::inf() : X[idx] * s2;
    }
}

template <typename T>
__global__ void k_cov_rows(T* sum, T hi, T lo) { sum[1] = hi; sum[2] = lo; }

}  // namespace mirlsq
