// spd_inverse_launch.h -- host view of the SPD inverse (spd_inverse.h): launch entry points, defined in launch_spd_inverse.hip,
// the translation unit that instantiates the kernels.
#pragma once

#include "common.h"

namespace mirlsq {

// elements of T the unit-level entries need as scratch: the n x n factor (L and its mirror) and the n scale factors behind it
inline size_t spd_inverse_work_elems(size_t n) { return n * n + n; }
// the widest matrix the column kernel takes: its vector of n elements lives in one workgroup's LDS (160 KB)
// (a limit of the layout, not a tested range: the tests go to n = 1024, the widest shape the solver itself is exercised at; the
// factor runs on ONE workgroup, so far above that a call takes seconds)
template <typename T> constexpr size_t spd_inverse_max_n() { return (size_t)160 * 1024 / sizeof(T); }

// X = inv(P): two launches on `s` (k_spd_factor, k_spd_columns), no synchronisation. P: n x n row-major, lower triangle read;
// fixed: n bytes or nullptr; W: n x n scratch (the factor); sv: n scratch (the scale factors); X: n x n; info: device int. All
// device pointers.
template <typename T>
hipError_t spd_inverse(int n, const T* P, const unsigned char* fixed, T* W, T* sv, T* X, int* info, hipStream_t s);

// cov = s^2 X (k_cov_scale): sum[0] = ||f||^2 on the device; rows_dev: the total row count is in sum[1], sum[2] (cov_rows)
template <typename T>
hipError_t cov_scale(int n, T* X, const unsigned char* fixed, const int* info, const T* sum, bool rows_dev, double rows_host,
                     double n_free, bool absolute, hipStream_t s);
// this rank's row count into sum[1], sum[2] as two exactly representable limbs (m / 4096, m % 4096): the all-reduce payload
template <typename T> hipError_t cov_rows(T* sum, size_t m, hipStream_t s);

}  // namespace mirlsq
