// launch_broyden.hip -- the translation unit that instantiates the read-only Broyden sweep and its companions
// (broyden_lr.h) and defines the launch entry points declared in broyden_launch.h.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "broyden_launch.h"
#include "launch_util.h"
#include "broyden_lr.h"

namespace mirlsq {

namespace {
// the one switch over lr_class(): f is called with the NCP and VEC of the instance as compile-time constants
template <typename F>
hipError_t lr_dispatch(LrClass c, F&& f)
{
#define MIRLSQ_LR_CASE(NCP)                                                                               \
    case NCP:                                                                                             \
        return c.vec ? f(std::integral_constant<int, NCP>{}, std::true_type{}) : f(std::integral_constant<int, NCP>{}, std::false_type{});
    switch (c.ncp) {
        MIRLSQ_LR_CASE(1)
        MIRLSQ_LR_CASE(2)
        MIRLSQ_LR_CASE(4)
        MIRLSQ_LR_CASE(8)
        MIRLSQ_LR_CASE(16)    // 256 < n <= 512: one workgroup a CU by registers, still one sweep over J
    }
#undef MIRLSQ_LR_CASE
    return hipErrorInvalidValue;
}
}  // namespace
template <typename T>
hipError_t lr_sweep(const LrArgs<T>& a, int nblk, hipStream_t s, const T* twh)
{
    if (a.n > kLrMaxN || a.k < 0 || a.k >= kLrMax) return hipErrorInvalidValue;
    if (twh) {
        // J is the unscaled difference panel: the scaled instance of the same class
        if constexpr (std::is_same<T, double>::value) {
            if (a.n > kLrScaledMaxN) return hipErrorInvalidValue;
            return lr_dispatch(lr_class_of<T>(a.n, a.J), [&](auto ncp, auto vec) {
                constexpr int NCP = decltype(ncp)::value;
                if constexpr (NCP <= kLrScaledMaxN / 32) {
                    MIRLSQ_LAUNCH((k_broyden_lr<T, NCP, decltype(vec)::value, const T*>), dim3(nblk), dim3(256), 0, s, a, twh);
                    return hipGetLastError();
                } else {
                    return hipErrorInvalidValue;
                }
            });
        } else {
            return hipErrorInvalidValue;                 // the difference panel exists in f64 only
        }
    }
    return lr_dispatch(lr_class_of<T>(a.n, a.J), [&](auto ncp, auto vec) {
        MIRLSQ_LAUNCH((k_broyden_lr<T, decltype(ncp)::value, decltype(vec)::value>), dim3(nblk), dim3(256), 0, s, a);
        return hipGetLastError();
    });
}

template <typename T>
hipError_t lr_flush(T* J, const T* U, const T* D, int k, size_t m, int n, int num_cu, hipStream_t s)
{
    if (k <= 0) return hipSuccess;
    if (n > kLrMaxN || k > kLrMax) return hipErrorInvalidValue;
    const size_t G = (m + 3) / 4;
    size_t blocks = (G + 3) / 4;
    if (blocks > (size_t)num_cu * 8) blocks = (size_t)num_cu * 8;
    if (blocks < 1) blocks = 1;
    const size_t lds = (size_t)k * n * sizeof(T);
    return lr_dispatch(lr_class_of<T>(n, J), [&](auto ncp, auto vec) {
        MIRLSQ_LAUNCH((k_lr_flush<T, decltype(ncp)::value, decltype(vec)::value>), dim3((unsigned)blocks), dim3(256), lds, s, J, U, D, k, m, n);
        return hipGetLastError();
    });
}

hipError_t lr_flush_scaled(double* J, const double* P, const double* twh, const double* U, const double* D, int k, size_t m, int n,
                           int num_cu, hipStream_t s)
{
    if (n > kLrScaledMaxN || k < 0 || k > kLrMax || !P || !twh) return hipErrorInvalidValue;
    const size_t G = (m + 3) / 4;
    size_t blocks = (G + 3) / 4;
    if (blocks > (size_t)num_cu * 8) blocks = (size_t)num_cu * 8;
    if (blocks < 1) blocks = 1;
    const size_t lds = (size_t)k * n * sizeof(double);
    const bool aligned = reinterpret_cast<uintptr_t>(J) % 16 == 0 && reinterpret_cast<uintptr_t>(P) % 16 == 0;
    return lr_dispatch(lr_class(n, aligned), [&](auto ncp, auto vec) {
        constexpr int NCP = decltype(ncp)::value;
        if constexpr (NCP <= kLrScaledMaxN / 32) {
            MIRLSQ_LAUNCH((k_lr_flush<double, NCP, decltype(vec)::value, LrFlushSrc<double>>), dim3((unsigned)blocks), dim3(256), lds, s, J, U, D, k, m, n,
                          LrFlushSrc<double>{P, twh});
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    });
}

template <typename T>
hipError_t lr_reduce(const T* partials, int nblk, int n, T* out, hipStream_t s)
{
    const int len = lr_len(n);
    MIRLSQ_LAUNCH(k_lr_reduce<T>, dim3((len + 31) / 32), dim3(32 * kReduceRanges), 0, s, partials, nblk, len, out);
    return hipGetLastError();
}

template <typename T>
hipError_t lr_finish(const T* lr, T* D, const T* dx, int k, int n, T* JJ, T* Jy, LmState<T>* st, hipStream_t s)
{
    MIRLSQ_LAUNCH(k_lr_finish<T>, dim3(n + 1), dim3(256), 0, s, lr, D, dx, k, n, JJ, Jy, st);
    return hipGetLastError();
}

template <typename T>
hipError_t lr_sumsq(const T* v, size_t m, int count, size_t vstride, T* partials, int pstride, int nblk, hipStream_t s)
{
    if (count < 1 || nblk < 1 || nblk > pstride) return hipErrorInvalidValue;
    MIRLSQ_LAUNCH(k_lr_sumsq<T>, dim3(nblk, count), dim3(256), 0, s, v, m, vstride, partials, pstride);
    return hipGetLastError();
}
template <typename T>
hipError_t lr_sumsq_final(const T* partials, int pstride, int nblk, int count, T* out, hipStream_t s)
{
    MIRLSQ_LAUNCH(k_lr_sumsq_final<T>, dim3(count), dim3(256), 0, s, partials, pstride, nblk, out);
    return hipGetLastError();
}

#define MIRLSQ_INSTANTIATE(T)                                                                                             \
    template hipError_t lr_sweep<T>(const LrArgs<T>&, int, hipStream_t, const T*);                                        \
    template hipError_t lr_reduce<T>(const T*, int, int, T*, hipStream_t);                                                \
    template hipError_t lr_finish<T>(const T*, T*, const T*, int, int, T*, T*, LmState<T>*, hipStream_t);                 \
    template hipError_t lr_sumsq<T>(const T*, size_t, int, size_t, T*, int, int, hipStream_t);                            \
    template hipError_t lr_sumsq_final<T>(const T*, int, int, int, T*, hipStream_t);                                      \
    template hipError_t lr_flush<T>(T*, const T*, const T*, int, size_t, int, int, hipStream_t);
MIRLSQ_INSTANTIATE(double)
MIRLSQ_INSTANTIATE(float)
#undef MIRLSQ_INSTANTIATE

}  // namespace mirlsq

MIRLSQ_DEFINE_PRELOAD(broyden)
