// solve_launch.h -- host view of the n x n kernels (solve_kernel.h / solve_lds.h for n <= 256, solve_big.h for any n):
// launch entry points, defined in launch_solve_d.hip / launch_solve_s.hip (one translation unit per element type: these
// kernels are the largest in the library). Argument blocks: solve_types.h.
// Reference operations replaced: least_squares.d:1053-1110, 1141-1142, 1164 and boxcqp.d:122-379 (solveBoxQP with
// mir-lapack's posvx('E','L')).
#pragma once

#include "common.h"
#include "solve_types.h"

namespace mirlsq {

// one workgroup per ladder entry (ks <= kChainMax). bounded = false: every lower / upper entry is infinite (the BOXCQP
// active-set loop is compiled out); generic = true: the any-n kernel of solve_big.h (required above n = kSolveMaxN)
template <typename T>
hipError_t launch_lm_solve(const LmSolveArgs<T>& a, int ks, bool bounded, bool generic, hipStream_t s);

// Which kernel launch_lm_solve runs, from (element size, n, bounded, generic, a diagnostic buffer in sc[0].dbg): the one
// statement of that choice (launch_lm_solve switches on it; mir_lsq_lm_solve_class exports it; host code, no device needed).
//   wave:      k_lm_solve_wave<bounded>             f64, n <= 16, no diagnostic buffer (solve_wave16.h)
//   workgroup: k_lm_solve<T, nb, bounded>           n <= kSolveMaxN; nb = solve_nb(n, elem): 1, 2, 4, 8 (factor in LDS) or 0
//   big:       k_lm_solve_big<T>                    generic, or n > kSolveMaxN; one instance a type (nb = 0, bounded = 1)
enum : int { kLmSolveWave = 0, kLmSolveWorkgroup = 1, kLmSolveBig = 2 };
constexpr int kSolveWaveMaxN = 16;       // == kW16 of solve_wave16.h (asserted where both are visible)
struct LmSolveClass { int kind, nb, bounded; };
inline LmSolveClass lm_solve_class(int elem, int n, bool bounded, bool generic, bool dbg)
{
    if (generic || n > kSolveMaxN) return {kLmSolveBig, 0, 1};
    if (elem == 8 && n <= kSolveWaveMaxN && !dbg) return {kLmSolveWave, 0, bounded ? 1 : 0};
    return {kLmSolveWorkgroup, solve_nb(n, elem), bounded ? 1 : 0};
}

// Workgroups per ladder entry of the any-n solve (LmSolveArgs::coop_w): with helpers, coop_peers(n) of them above n = kSolveMaxN.
// An entry's workgroups hold a CU each (150 KB of LDS) and wait for one another: never more of them than half the device (a
// partitioned or masked GPU), or a group could never be resident at once.
inline int coop_width(int n, int num_cu, bool helpers)
{
    int w = (helpers && n > kSolveMaxN) ? coop_peers(n) : 1;
    if (w > num_cu / 2) w = num_cu / 2 >= 2 ? num_cu / 2 : 1;
    return w;
}

// standalone BOXCQP on device-resident operands (mir_solve_box_qp_gpu_*): picks the kernel by a.n
template <typename T>
hipError_t launch_box_qp(const BoxQpArgs<T>& a, hipStream_t s);

}  // namespace mirlsq
