// launch_spd_inverse.hip -- the translation unit that instantiates the SPD inverse (spd_inverse.h), defines the launch entry
// points of spd_inverse_launch.h and the unit-level C entries mir_lsq_spd_inverse_* (include/mir_optim_amd.h).
#include <hip/hip_runtime.h>

#include "../../include/mir_optim_amd.h"
#include "launch_util.h"
#include "spd_inverse.h"
#include "spd_inverse_launch.h"

namespace mirlsq {

bool device_available();       // workspace.hip

template <typename T>
hipError_t spd_inverse(int n, const T* P, const unsigned char* fixed, T* W, T* sv, T* X, int* info, hipStream_t s)
{
    if (n < 1 || (size_t)n > spd_inverse_max_n<T>() || !P || !W || !sv || !X || !info) return hipErrorInvalidValue;
    const size_t lds = (size_t)n * sizeof(T);
    MIRLSQ_ENSURE_LDS(k_spd_columns<T>, lds);
    MIRLSQ_LAUNCH(k_spd_factor<T>, dim3(1), dim3(kInvThreads), 0, s, n, P, fixed, W, sv, info);
    MIRLSQ_LAUNCH(k_spd_columns<T>, dim3(n), dim3(kWave), lds, s, n, W, sv, fixed, info, X);
    return hipGetLastError();
}

template <typename T>
hipError_t cov_scale(int n, T* X, const unsigned char* fixed, const int* info, const T* sum, bool rows_dev, double rows_host,
                     double n_free, bool absolute, hipStream_t s)
{
    size_t blocks = ((size_t)n * n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    MIRLSQ_LAUNCH(k_cov_scale<T>, dim3((unsigned)blocks), dim3(256), 0, s, n, X, fixed, info, sum, rows_dev ? 1 : 0, rows_host,
                  n_free, absolute ? 1 : 0);
    return hipGetLastError();
}

template <typename T>
hipError_t cov_rows(T* sum, size_t m, hipStream_t s)
{
    MIRLSQ_LAUNCH(k_cov_rows<T>, dim3(1), dim3(1), 0, s, sum, (T)(m / 4096), (T)(m % 4096));
    return hipGetLastError();
}

#define MIRLSQ_INSTANTIATE(T)                                                                                             \
    template hipError_t spd_inverse<T>(int, const T*, const unsigned char*, T*, T*, T*, int*, hipStream_t);                   \
    template hipError_t cov_scale<T>(int, T*, const unsigned char*, const int*, const T*, bool, double, double, bool, hipStream_t); \
    template hipError_t cov_rows<T>(T*, size_t, hipStream_t);
MIRLSQ_INSTANTIATE(double)
MIRLSQ_INSTANTIATE(float)
#undef MIRLSQ_INSTANTIATE

namespace {
// the entry with caller-owned scratch: enqueues and returns
template <typename T>
int spd_inverse_work_entry(size_t n, const T* P, const unsigned char* fixed, T* X, int* info, void* work, size_t work_bytes,
                           void* stream)
{
    if (n == 0 || n > spd_inverse_max_n<T>() || !P || !X || !info || !work) return -1;
    if (work_bytes < spd_inverse_work_elems(n) * sizeof(T)) return -1;
    if (!device_available()) return -2;
    T* W = static_cast<T*>(work);
    return spd_inverse<T>((int)n, P, fixed, W, W + n * n, X, info, static_cast<hipStream_t>(stream)) == hipSuccess ? 0 : -4;
}
// the entry that owns its scratch: synchronises before it returns (as mir_lsq_jtj_*)
template <typename T>
int spd_inverse_entry(size_t n, const T* P, const unsigned char* fixed, T* X, int* info, void* stream)
{
    if (n == 0 || n > spd_inverse_max_n<T>() || !P || !X || !info) return -1;
    if (!device_available()) return -2;
    void* work = nullptr;
    const size_t bytes = spd_inverse_work_elems(n) * sizeof(T);
    if (hipMalloc(&work, bytes) != hipSuccess) return -3;
    int rc = spd_inverse_work_entry<T>(n, P, fixed, X, info, work, bytes, stream);
    if (hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess && rc == 0) rc = -5;
    (void)hipFree(work);
    return rc;
}
}  // namespace

}  // namespace mirlsq

extern "C" {

int mir_lsq_spd_inverse_d(size_t n, const double* P, const unsigned char* fixed, double* X, int* info, void* stream)
{
    return mirlsq::spd_inverse_entry<double>(n, P, fixed, X, info, stream);
}
int mir_lsq_spd_inverse_s(size_t n, const float* P, const unsigned char* fixed, float* X, int* info, void* stream)
{
    return mirlsq::spd_inverse_entry<float>(n, P, fixed, X, info, stream);
}
size_t mir_lsq_spd_inverse_work_bytes(size_t n, size_t elem_size)
{
    return (elem_size == 4 || elem_size == 8) ? mirlsq::spd_inverse_work_elems(n) * elem_size : 0;
}
int mir_lsq_spd_inverse_work_d(size_t n, const double* P, const unsigned char* fixed, double* X, int* info, void* work,
                               size_t work_bytes, void* stream)
{
    return mirlsq::spd_inverse_work_entry<double>(n, P, fixed, X, info, work, work_bytes, stream);
}
int mir_lsq_spd_inverse_work_s(size_t n, const float* P, const unsigned char* fixed, float* X, int* info, void* work,
                               size_t work_bytes, void* stream)
{
    return mirlsq::spd_inverse_work_entry<float>(n, P, fixed, X, info, work, work_bytes, stream);
}

}  // extern "C"
