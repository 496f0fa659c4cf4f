// spline_c2.h -- ONE statement of the arithmetic of fit_spline.cpp (c2_not_a_knot, hermite_eval, the penalty of
// fit_residuals) for host and device, split so that what depends only on the knots is computed once per fit and what
// depends on a value vector once per vector, and the per-row work is a table look-up and one Horner form.
//
// Every function restates fit_spline.cpp operation for operation (the line numbers cited are that file's): the same
// + - * / sqrt in the same order on the same operands, with contraction off, so the results are the bits of fit_spline.cpp
// wherever those operations are correctly rounded (tests/test_fit_spline_gpu_host.py holds the host instance to that with
// array_equal, tests/test_gpu_fit_spline.py the kernels to the host instance). No fast-math, no reciprocals.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SPLINE_HD __host__ __device__ inline
#else
#define SPLINE_HD inline
#endif

namespace spline_c2 {

// The factor of the not-a-knot system (n >= 4): 5 n values, [di | up | up2 | f | swap] -- the three diagonals AFTER the
// elimination of lines 64-75, the multiplier f of every step and its pivot decision (1 = the rows were swapped). n < 4 has
// no system (closed forms): the factor is not read.
constexpr size_t kFactorArrays = 5;
template <typename T> struct Factor {
    const T *di, *up, *up2, *f, *swp;
    SPLINE_HD Factor(const T* F, size_t n) : di(F), up(F + n), up2(F + 2 * n), f(F + 3 * n), swp(F + 4 * n) {}
};

// lines 43-75 without r: `work` holds n values (the sub-diagonal lo)
template <typename T>
SPLINE_HD void c2_factor(size_t n, const T* x, T* F, T* work)
{
#pragma clang fp contract(off)
    for (size_t i = 0; i < kFactorArrays * n; ++i) F[i] = 0;
    if (n < 4) return;
    T *di = F, *up = F + n, *up2 = F + 2 * n, *f = F + 3 * n, *swp = F + 4 * n, *lo = work;
    auto h = [&](size_t i) { return x[i + 1] - x[i]; };
    for (size_t i = 1; i + 1 < n; ++i) {
        lo[i] = h(i);
        di[i] = 2 * (h(i - 1) + h(i));
        up[i] = h(i - 1);
    }
    {
        const T h0 = h(0), h1 = h(1);
        lo[0] = 0; di[0] = h1; up[0] = h0 + h1;
    }
    {
        const T ha = h(n - 2), hb = h(n - 3);
        lo[n - 1] = ha + hb; di[n - 1] = hb; up[n - 1] = 0;
    }
    for (size_t i = 0; i + 1 < n; ++i) {
        if (std::fabs(lo[i + 1]) > std::fabs(di[i])) {
            T t;
            t = di[i]; di[i] = lo[i + 1]; lo[i + 1] = t;
            t = up[i]; up[i] = di[i + 1]; di[i + 1] = t;
            t = up2[i]; up2[i] = up[i + 1]; up[i + 1] = t;
            swp[i] = 1;
        }
        f[i] = lo[i + 1] / di[i];
        di[i + 1] -= f[i] * up[i];
        up[i + 1] -= f[i] * up2[i];
    }
}

// First derivatives d of the spline with values y: the bits of c2_not_a_knot. h[i] = x[i + 1] - x[i] (n - 1 values); d is
// also the right-hand side's storage (r[k] is read before d[k] is written, d[k + 1] and d[k + 2] are final by then).
template <typename T>
SPLINE_HD void c2_solve(size_t n, const T* h, const T* F, const T* y, T* d)
{
#pragma clang fp contract(off)
    if (n == 0) return;
    if (n == 1) { d[0] = 0; return; }
    if (n == 2) { d[0] = d[1] = (y[1] - y[0]) / h[0]; return; }
    if (n == 3) {
        const T h0 = h[0], h1 = h[1];
        const T s0 = (y[1] - y[0]) / h0, s1 = (y[2] - y[1]) / h1;
        const T c = (s1 - s0) / (h0 + h1);
        d[0] = s0 - c * h0;
        d[1] = s0 + c * h0;
        d[2] = s1 + c * h1;
        return;
    }
    const Factor<T> K(F, n);
    T* r = d;
    auto s = [&](size_t i) { return (y[i + 1] - y[i]) / h[i]; };
    for (size_t i = 1; i + 1 < n; ++i) r[i] = 3 * (h[i] * s(i - 1) + h[i - 1] * s(i));                // line 50
    {
        const T h0 = h[0], h1 = h[1];
        r[0] = ((3 * h0 + 2 * h1) * h1 * s(0) + h0 * h0 * s(1)) / (h0 + h1);                          // line 55
    }
    {
        const T ha = h[n - 2], hb = h[n - 3];
        r[n - 1] = (ha * ha * s(n - 3) + (2 * hb + 3 * ha) * hb * s(n - 2)) / (ha + hb);              // line 60
    }
    for (size_t i = 0; i + 1 < n; ++i) {
        if (K.swp[i] != 0) { const T t = r[i]; r[i] = r[i + 1]; r[i + 1] = t; }                      // line 69
        r[i + 1] -= K.f[i] * r[i];                                                                    // line 74
    }
    d[n - 1] = r[n - 1] / K.di[n - 1];                                                                // lines 76-78
    d[n - 2] = (r[n - 2] - K.up[n - 2] * d[n - 1]) / K.di[n - 2];
    for (size_t k = n - 2; k-- > 0;) d[k] = (r[k] - K.up[k] * d[k + 1] - K.up2[k] * d[k + 2]) / K.di[k];
}

// {y0, d0, c2, c3} of interval lo (lines 94-96); n == 1 has no interval: the constant y[0]
template <typename T>
SPLINE_HD void segment_coeffs(size_t n, const T* h, const T* y, const T* d, size_t lo, T out[4])
{
#pragma clang fp contract(off)
    if (n < 2) { out[0] = n ? y[0] : T(0); out[1] = out[2] = out[3] = 0; return; }
    const T s = (y[lo + 1] - y[lo]) / h[lo];
    out[0] = y[lo];
    out[1] = d[lo];
    out[2] = 3 * s - 2 * d[lo] - d[lo + 1];
    out[3] = d[lo] + d[lo + 1] - 2 * s;
}

// the interval of t (lines 87-91, verbatim) and u = (t - x[lo]) / h (lines 92-93); n < 2: interval 0, u = 0
template <typename T>
SPLINE_HD void row_locate(size_t n, const T* x, T t, int32_t* seg, T* u)
{
#pragma clang fp contract(off)
    if (n < 2) { *seg = 0; *u = 0; return; }
    size_t lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) / 2;
        if (t < x[mid]) hi = mid; else lo = mid;
    }
    const T h = x[lo + 1] - x[lo];
    *seg = (int32_t)lo;
    *u = (t - x[lo]) / h;
}

// line 97. n == 1 is served with h = 0, u = 0 and {y0, 0, 0, 0}
template <typename T>
SPLINE_HD T segment_value(T y0, T d0, T c2, T c3, T h, T u)
{
#pragma clang fp contract(off)
    return y0 + h * u * (d0 + u * (c2 + u * c3));
}

// lines 123-132
template <typename T>
SPLINE_HD T penalty(size_t n, const T* x, const T* d, T lambda, size_t np)
{
#pragma clang fp contract(off)
    T integral = 0;
    if (lambda != 0) {
        T ld = d[0];
        for (size_t i = 1; i < n; ++i) {
            const T rd = d[i];
            integral += (rd * rd + rd * ld + ld * ld) * (x[i] - x[i - 1]);
            ld = rd;
        }
    }
    return std::sqrt(integral * lambda * (T)np / (T)(3 * n));
}

}  // namespace spline_c2
