// fit_spline_kernels.h -- the residuals of fitSpline (fit_spline.cpp: fit_residuals) as kernels, for the device-callback
// contract of the solver (f, fb, fbRowMajorDiff with MIR_LSQ_FD_BASE_POINT). The arithmetic is spline_c2.h's.
//
//   once per fit      k_spline_rows    per point: interval (int32) and u = (t - x_lo) / h: the hot sweeps never search
//   per callback      k_spline_tables  one wave per parameter vector: first derivatives (serial, in LDS), then the table
//                                      C[seg][k] = {y0, d0, c2, c3} ((nx - 1) x p entries, the p vectors' entries of one
//                                      interval contiguous) and pen[k]
//                     k_spline_points  Y[k m + i] (point-major): lanes across rows
//                     k_spline_diff    D[i nx + j] = r(X_2j)_i - r(X_2j+1)_i (row-major): lanes across columns; with
//                                      p = 2 nx + 1 the residual vector of the last point behind the panel
// Row i < m - 1 is value - data_i, row m - 1 is always pen[k] (fit_spline.cpp line 132: with lambda != 0 it replaces the last
// point). The host_* functions run the same statements on the CPU (mir_fit_spline_eval_host_*).
#pragma once

#include <hip/hip_runtime.h>

#include "spline_c2.h"

namespace spline_gpu {

constexpr int kWaveLanes = 64;
constexpr int kBlock = 256;
constexpr int kDiffSteps = 8;   // row groups a workgroup of k_spline_diff walks

// residual of a point row from one table entry: the ONE statement behind k_spline_points, k_spline_diff and the host twins
template <typename T>
SPLINE_HD T row_residual(const T* c, T h, T u, T data)
{
#pragma clang fp contract(off)
    return spline_c2::segment_value(c[0], c[1], c[2], c[3], h, u) - data;
}
template <typename T>
SPLINE_HD T row_value(const T* c, T h, T u)
{
#pragma clang fp contract(off)
    return spline_c2::segment_value(c[0], c[1], c[2], c[3], h, u);
}

// table + penalty of ONE value vector y (d: nx values of work space, the derivatives on return); C is the table of p vectors,
// this one is vector k
template <typename T>
SPLINE_HD void vector_tables(size_t nx, const T* x, const T* h, const T* F, const T* y, T* d, T lambda, size_t np, size_t p,
                             size_t k, T* C, T* pen)
{
    spline_c2::c2_solve(nx, h, F, y, d);
    const size_t nseg = nx > 1 ? nx - 1 : 1;
    for (size_t s = 0; s < nseg; ++s) spline_c2::segment_coeffs(nx, h, y, d, s, C + (s * p + k) * 4);
    pen[k] = spline_c2::penalty(nx, x, d, lambda, np);
}

// t = tp[i * stride] (points: stride 2; a plain abscissa array: stride 1)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_spline_rows(size_t count, const T* tp, size_t stride, size_t nx, const T* x,
                                                        int32_t* seg, T* u)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    int32_t s; T uu;
    spline_c2::row_locate(nx, x, tp[i * stride], &s, &uu);
    seg[i] = s;
    u[i] = uu;
}

// One wave per vector. LDS (staged != 0): y, d, h, x (nx each) and the factor (5 nx): 9 nx values, so that the serial solve of
// lane 0 waits for LDS and not for HBM. Knot counts whose 9 nx values do not fit (staged == 0) read the inputs from global
// memory and keep d in dwork (p x nx).
template <typename T>
__global__ __launch_bounds__(kWaveLanes) void k_spline_tables(size_t nx, size_t p, const T* X, const T* x, const T* h,
                                                              const T* F, T lambda, size_t np, T* C, T* pen, T* dwork,
                                                              int staged)
{
#pragma clang fp contract(off)
    extern __shared__ double lds_raw[];
    const size_t k = blockIdx.x;
    const int lane = threadIdx.x;
    const T *yy = X + k * nx, *xx = x, *hh = h, *FF = F;
    T* d;
    if (staged) {
        T* L = reinterpret_cast<T*>(lds_raw);
        T *ly = L, *ld = L + nx, *lh = L + 2 * nx, *lx = L + 3 * nx, *lF = L + 4 * nx;
        for (size_t i = lane; i < nx; i += kWaveLanes) { ly[i] = yy[i]; lx[i] = x[i]; lh[i] = i + 1 < nx ? h[i] : T(0); }
        for (size_t i = lane; i < spline_c2::kFactorArrays * nx; i += kWaveLanes) lF[i] = F[i];
        yy = ly; xx = lx; hh = lh; FF = lF; d = ld;
    } else {
        d = dwork + k * nx;
    }
    __syncthreads();
    if (lane == 0) {
        spline_c2::c2_solve(nx, hh, FF, yy, d);
        pen[k] = spline_c2::penalty(nx, xx, d, lambda, np);
    }
    __syncthreads();
    const size_t nseg = nx > 1 ? nx - 1 : 1;
    for (size_t s = lane; s < nseg; s += kWaveLanes) spline_c2::segment_coeffs(nx, hh, yy, d, s, C + (s * p + k) * 4);
}

// Y[k * m + i], i < m: rows < m - 1 (all rows when pen == nullptr) are point rows, row m - 1 is pen[k]. points == nullptr:
// values only (data 0 is not subtracted: mir_spline_eval_gpu_*). grid = (row blocks, p)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_spline_points(size_t m, size_t p, const int32_t* seg, const T* u, const T* h,
                                                          const T* C, const T* pen, const T* points, T* Y)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t k = blockIdx.y;
    if (i >= m) return;
    T v;
    if (pen && i == m - 1) {
        v = pen[k];
    } else {
        const size_t s = (size_t)seg[i];
        const T* c = C + (s * p + k) * 4;
        v = points ? row_residual(c, h[s], u[i], points[2 * i + 1]) : row_value(c, h[s], u[i]);
    }
    Y[k * m + i] = v;
}

// D[i * nx + j] = r(X_2j)_i - r(X_2j+1)_i; p = 2 nx or 2 nx + 1 (then also D[m nx + i] = r(X_2nx)_i). W lanes (a power of two,
// <= 64) walk the columns of a row, kBlock / W rows at a time: a lane reads the two table entries of its column pair as 8
// contiguous values and the W lanes of a row store W contiguous values of the panel.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_spline_diff(size_t m, size_t nx, size_t p, int W, const int32_t* seg, const T* u,
                                                        const T* h, const T* C, const T* pen, const T* points, T* D)
{
#pragma clang fp contract(off)
    const int rows = kBlock / W;
    const int rl = threadIdx.x / W, c0 = threadIdx.x % W;
    const bool base = p == 2 * nx + 1;
    for (int step = 0; step < kDiffSteps; ++step) {
        const size_t i = ((size_t)blockIdx.x * kDiffSteps + step) * rows + rl;
        if (i >= m) return;
        if (i == m - 1) {
            for (size_t j = c0; j < nx; j += W) D[i * nx + j] = pen[2 * j] - pen[2 * j + 1];
            if (base && c0 == 0) D[m * nx + i] = pen[2 * nx];
            continue;
        }
        const size_t s = (size_t)seg[i];
        const T ui = u[i], hs = h[s], data = points[2 * i + 1];
        const T* Cs = C + s * p * 4;
        for (size_t j = c0; j < nx; j += W) {
            const T* c = Cs + 8 * j;
            const T rp = row_residual(c, hs, ui, data);
            const T rm = row_residual(c + 4, hs, ui, data);
            D[i * nx + j] = rp - rm;
        }
        if (base && c0 == 0) D[m * nx + i] = row_residual(Cs + 8 * nx, hs, ui, data);
    }
}

// ---- the same statements on the host
template <typename T>
void host_rows(size_t count, const T* tp, size_t stride, size_t nx, const T* x, int32_t* seg, T* u)
{
    for (size_t i = 0; i < count; ++i) spline_c2::row_locate(nx, x, tp[i * stride], seg + i, u + i);
}
template <typename T>
void host_points(size_t m, size_t p, const int32_t* seg, const T* u, const T* h, const T* C, const T* pen, const T* points, T* Y)
{
    for (size_t k = 0; k < p; ++k)
        for (size_t i = 0; i < m; ++i) {
            if (i == m - 1) { Y[k * m + i] = pen[k]; continue; }
            const size_t s = (size_t)seg[i];
            Y[k * m + i] = row_residual(C + (s * p + k) * 4, h[s], u[i], points[2 * i + 1]);
        }
}
template <typename T>
void host_diff(size_t m, size_t nx, size_t p, const int32_t* seg, const T* u, const T* h, const T* C, const T* pen,
               const T* points, T* D)
{
    const bool base = p == 2 * nx + 1;
    for (size_t i = 0; i < m; ++i) {
        if (i == m - 1) {
            for (size_t j = 0; j < nx; ++j) D[i * nx + j] = pen[2 * j] - pen[2 * j + 1];
            if (base) D[m * nx + i] = pen[2 * nx];
            continue;
        }
        const size_t s = (size_t)seg[i];
        const T* Cs = C + s * p * 4;
        for (size_t j = 0; j < nx; ++j) {
            const T rp = row_residual(Cs + 8 * j, h[s], u[i], points[2 * i + 1]);
            const T rm = row_residual(Cs + 8 * j + 4, h[s], u[i], points[2 * i + 1]);
            D[i * nx + j] = rp - rm;
        }
        if (base) D[m * nx + i] = row_residual(Cs + 8 * nx, h[s], u[i], points[2 * i + 1]);
    }
}

}  // namespace spline_gpu
