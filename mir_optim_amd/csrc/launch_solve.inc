// launch_solve.inc -- body of launch_solve_d.hip / launch_solve_s.hip (MIRLSQ_SOLVE_T = double / float)
#include <hip/hip_runtime.h>

#include <type_traits>

#include "launch_util.h"
#include "solve_launch.h"
#include "solve_kernel.h"
#include "solve_big.h"

namespace mirlsq {

namespace {
template <typename T, int NB, bool BOUNDED>
hipError_t lm_solve_nbb(const LmSolveArgs<T>& a, int ks, size_t lds, hipStream_t s)
{
    auto kern = k_lm_solve<T, NB, BOUNDED>;
    if (lds > 48 * 1024) MIRLSQ_ENSURE_LDS(kern, (size_t)kSolveLdsBytes);   // (+ the kernel's static variables: under the CU's 160 KB)
    MIRLSQ_LAUNCH(kern, dim3(ks), dim3(kSolveThreads), lds, s, a);
    return hipGetLastError();
}
template <typename T, int NB>
hipError_t lm_solve_nb(const LmSolveArgs<T>& a, int ks, bool bounded, size_t lds, hipStream_t s)
{
    return bounded ? lm_solve_nbb<T, NB, true>(a, ks, lds, s) : lm_solve_nbb<T, NB, false>(a, ks, lds, s);
}
template <typename T, int NB>
hipError_t box_qp_nb(const BoxQpArgs<T>& a, size_t lds, hipStream_t s)
{
    auto kern = k_box_qp<T, NB>;
    if (lds > 48 * 1024) MIRLSQ_ENSURE_LDS(kern, (size_t)kSolveLdsBytes);   // (+ the kernel's static variables: under the CU's 160 KB)
    MIRLSQ_LAUNCH(kern, dim3(1), dim3(kSolveThreads), lds, s, a);
    return hipGetLastError();
}
}  // namespace

template <typename T>
hipError_t launch_lm_solve(const LmSolveArgs<T>& a, int ks, bool bounded, bool generic, hipStream_t s)
{
    if (ks < 1 || ks > kChainMax) return hipErrorInvalidValue;
    if (a.fused && (generic || a.n > kSolveMaxN || ks != 1)) return hipErrorInvalidValue;   // fused rounds: the one-workgroup kernels
    static_assert(kSolveWaveMaxN == kW16, "lm_solve_class sends n <= kSolveWaveMaxN to the kernel compiled for kW16 rows");
    const LmSolveClass cls = lm_solve_class((int)sizeof(T), a.n, bounded, generic, a.sc[0].dbg != nullptr);
    if (cls.kind == kLmSolveBig) {
        // any n: one 512-thread workgroup per ladder entry, matrices in global memory (solve_big.h)
        // (a.coop_w > 1: coop_w workgroups per entry, the first of each group is the entry's own -- solve_coop.h)
        auto kern = k_lm_solve_big<T>;
        const int w = (a.coop_w > 1 && a.sc[0].coop && a.sc[0].cS) ? a.coop_w : 1;
        if (w > kCoopMaxPeers) return hipErrorInvalidValue;
        MIRLSQ_ENSURE_LDS(kern, sizeof(BigLds<T>));
        LmSolveArgs<T> a2 = a;                               // the kernel derives its groups from coop_w: the width the grid is sized with
        a2.coop_w = w;
        if (w == 1) a2.coop_epoch = 0;
        if (a.coop_absent && w > 1) {
            // diagnostic: the kernel indexes its entries by blockIdx / coop_w, so the mains are launched ONE entry at a time here
            // (entry kc's main is block kc * w of a grid that ends right behind it)
            if (ks != 1) return hipErrorInvalidValue;
            MIRLSQ_LAUNCH(kern, dim3(1), dim3(kBigThreads), sizeof(BigLds<T>), s, a2);
        } else {
            MIRLSQ_LAUNCH(kern, dim3(ks * w), dim3(kBigThreads), sizeof(BigLds<T>), s, a2);
        }
        if (w > 1) {
            // the RESCUE launch: entries whose helpers did not answer in time are solved again on one workgroup -- behind the
            // kernel boundary, when every workgroup of the launch above (late helpers too) has ended; all others return at once
            a2.coop_w = 1; a2.coop_epoch = 0; a2.coop_rescue = 1;
            MIRLSQ_LAUNCH(kern, dim3(ks), dim3(kBigThreads), sizeof(BigLds<T>), s, a2);
        }
        return hipGetLastError();
    }
    if constexpr (std::is_same<T, double>::value) {
        // n <= 16: one wave per ladder entry, a matrix row per lane (solve_wave16.h). (The phase stamps of DEBUG_SOLVE belong to
        // the workgroup kernel: a diagnostic run keeps it.)
        if (cls.kind == kLmSolveWave) {
            if (bounded) MIRLSQ_LAUNCH(k_lm_solve_wave<true>, dim3(ks), dim3(kWave), 0, s, a);
            else MIRLSQ_LAUNCH(k_lm_solve_wave<false>, dim3(ks), dim3(kWave), 0, s, a);
            return hipGetLastError();
        }
    }
    const size_t lds = solve_lds_bytes(a.n, (int)sizeof(T));
    switch (cls.nb) {
    case 1: return lm_solve_nb<T, 1>(a, ks, bounded, lds, s);
    case 2: return lm_solve_nb<T, 2>(a, ks, bounded, lds, s);
    case 4: return lm_solve_nb<T, 4>(a, ks, bounded, lds, s);
    case 8: return lm_solve_nb<T, 8>(a, ks, bounded, lds, s);
    default: return lm_solve_nb<T, 0>(a, ks, bounded, lds, s);
    }
}

template <typename T>
hipError_t launch_box_qp(const BoxQpArgs<T>& a, hipStream_t s)
{
    if (a.n > kSolveMaxN) {
        auto kern = k_box_qp_big<T>;
        MIRLSQ_ENSURE_LDS(kern, sizeof(BigLds<T>));
        MIRLSQ_LAUNCH(kern, dim3(1), dim3(kBigThreads), sizeof(BigLds<T>), s, a);
        return hipGetLastError();
    }
    const size_t lds = solve_lds_bytes(a.n, (int)sizeof(T));
    switch (solve_nb(a.n, (int)sizeof(T))) {
    case 1: return box_qp_nb<T, 1>(a, lds, s);
    case 2: return box_qp_nb<T, 2>(a, lds, s);
    case 4: return box_qp_nb<T, 4>(a, lds, s);
    case 8: return box_qp_nb<T, 8>(a, lds, s);
    default: return box_qp_nb<T, 0>(a, lds, s);
    }
}

template hipError_t launch_lm_solve<MIRLSQ_SOLVE_T>(const LmSolveArgs<MIRLSQ_SOLVE_T>&, int, bool, bool, hipStream_t);
template hipError_t launch_box_qp<MIRLSQ_SOLVE_T>(const BoxQpArgs<MIRLSQ_SOLVE_T>&, hipStream_t);

}  // namespace mirlsq

#define MIRLSQ_PRELOAD_CAT2(a) MIRLSQ_DEFINE_PRELOAD(a)
MIRLSQ_PRELOAD_CAT2(MIRLSQ_SOLVE_TAG)
