// fit_spline_gpu.h -- what fit_spline_gpu.hip offers the unit-level entries of unit_entries.hip (mir_fit_spline_gpu_eval_*,
// mir_fit_spline_eval_host_*, mir_fit_spline_factor_*). Instantiated for double and float in fit_spline_gpu.hip.
#pragma once

#include <cstddef>

namespace spline_gpu {

// The per-fit setup of mir_fit_spline_gpu_* and then exactly the callback a solve would call on X (p x nx, HOST; uploaded):
// mode 0 = fb -> out p x m point-major, mode 1 = fbRowMajorDiff (double; p = 2 nx or 2 nx + 1) -> out m nx (+ m). points:
// DEVICE, npoints x 2. 0, or -1 arguments, -2 no device, -3 allocation, -5 a launch or copy failed.
template <typename T>
int callback_eval(size_t npoints, const T* points_dev, size_t nx, const T* x, T lambda, size_t p, const T* X_host, int mode,
                  T* out_host);
// the same two stages of spline_c2.h on the CPU (points: HOST); mode 1 in either precision
template <typename T>
int host_eval(size_t npoints, const T* points, size_t nx, const T* x, T lambda, size_t p, const T* X_host, int mode, T* out_host);
// the factor of the knots as the callbacks use it: F[5 nx] = [di | up | up2 | f | swap] (all 0 for nx < 4)
template <typename T>
int factor(size_t nx, const T* x, T* F);

}  // namespace spline_gpu
