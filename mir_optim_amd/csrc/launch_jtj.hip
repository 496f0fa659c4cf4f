// launch_jtj.hip -- the ONE translation unit that instantiates the J^T J kernels (jtj_kernel.h, jtj_fdp.h, jtj_fdp8.h,
// jtj_pc32.h, jtj_ring8.h, jtj_wide.h) and defines the launch entry point declared in jtj_plan.h.
// Reference operations replaced: least_squares.d:1052 (gemv J^T y), 1065 (syrk J^T J), 1041-1047 (finite-difference column
// arithmetic, fused), and -- MIR_LSQ_VARIANT_BROYDEN_REWRITE only -- 1003-1006 (Broyden update with J rewritten).
#include <hip/hip_runtime.h>

#include "jtj_plan.h"
#include "launch_util.h"
#include "solve_types.h"
#include "jtj_kernel.h"
#include "jtj_fdp.h"
#include "jtj_fdp8.h"
#include "jtj_pc32.h"
#include "jtj_ring8.h"
#include "jtj_wide.h"
#include "misc_kernels.h"

namespace mirlsq {

namespace {

// a run-time block count in {LO, LO + STEP, .. HI} -> f(std::integral_constant<int, NCB>); outside of it: hipErrorInvalidValue
template <int LO, int HI, int STEP = 1, typename F>
hipError_t dispatch_ncb(int ncb, F&& f)
{
    if constexpr (LO > HI) return hipErrorInvalidValue;
    else return ncb == LO ? f(std::integral_constant<int, LO>{}) : dispatch_ncb<LO + STEP, HI, STEP>(ncb, f);
}

// one kernel on the grid and with the dynamic LDS of its plan entry
template <auto Kern, typename... A>
hipError_t launch_one(const JtjLaunch& l, int threads, hipStream_t s, const A&... args)
{
    MIRLSQ_ENSURE_LDS(Kern, l.lds);
    MIRLSQ_LAUNCH(Kern, dim3(l.nblk, l.njobs), dim3(threads), l.lds, s, args...);
    return hipGetLastError();
}

// k_jtj_fdp (jtj_fdp.h); FD: the finite-difference pair panel is the source, DIFF: the difference panel
template <int NCB, bool FD, bool DIFF>
hipError_t fdp_one(const JtjLaunch& l, const JtjArgs<double>& a, hipStream_t s)
{
    using FC = JtjFdpCfg<NCB, FD>;
    static_assert(jtj_fdp_lds_bytes(NCB, FD) == FC::LDS_BYTES && jtj_fdp_flat_bytes(NCB) == FC::N * sizeof(double), "jtj_plan.h: k_jtj_fdp LDS size");
    static_assert(JtjFdpCfg<NCB, false>::RS == kJtjFdpStageRows, "jtj_plan.h: the stage of the 4 GB rule of fd_diff_keep");
    if constexpr (!FD) if (l.flat) return launch_one<k_jtj_fdp<NCB, FD, DIFF, true>>(l, FC::THREADS, s, a);
    return launch_one<k_jtj_fdp<NCB, FD, DIFF>>(l, FC::THREADS, s, a);
}
// k_jtj_fdp8 (jtj_fdp8.h); PLAIN: J^T J of a given J
template <int NCB, bool DIFF, bool PLAIN>
hipError_t fdp8_one(const JtjLaunch& l, const JtjArgs<double>& a, hipStream_t s)
{
    static_assert(jtj_fdp8_lds_bytes(NCB) == JtjFdp8Cfg<NCB>::LDS_BYTES, "jtj_plan.h: k_jtj_fdp8 LDS size");
    return launch_one<k_jtj_fdp8<NCB, DIFF, PLAIN>>(l, JtjFdp8Cfg<NCB>::THREADS, s, a);
}

// the kernel of a resolved plan entry; the instantiated block counts are the ranges of the dispatch_ncb calls
template <typename T>
hipError_t launch_kernel(const JtjLaunch& l, JtjOp op, const JtjArgs<T>& a, hipStream_t s)
{
    constexpr bool f64 = sizeof(T) == 8;
    const bool rewrite = op == JtjOp::rewrite, diff = op == JtjOp::fd_diff || op == JtjOp::fd_diff_keep;
    switch (l.kernel) {
    case JtjKernel::stream:
        return dispatch_ncb<1, 8>(l.ncb, [&](auto NCB) {
            if (rewrite) return launch_one<k_jtj<T, NCB, true>>(l, 256, s, a);
            if constexpr (!f64) return launch_one<k_jtj<T, NCB, false>>(l, 256, s, a);
            return hipErrorInvalidValue;                   // f64: every plain product at n <= 128 is k_jtj_fdp's
        });
    case JtjKernel::fdp:
        if constexpr (f64) return dispatch_ncb<1, 8>(l.ncb, [&](auto NCB) {
            return op == JtjOp::fd ? fdp_one<NCB, true, false>(l, a, s)
                 : (diff ? fdp_one<NCB, false, true>(l, a, s) : fdp_one<NCB, false, false>(l, a, s));
        });
        break;
    case JtjKernel::fdp_nw:                                // fdp's store-free instance (fd_diff_keep): the plan entry is fdp's
        if constexpr (f64) return dispatch_ncb<1, 8>(l.ncb, [&](auto NCB) {
            return launch_one<k_jtj_fdp_nw<NCB>>(l, JtjFdpCfg<NCB, false>::THREADS, s, a);
        });
        break;
    case JtjKernel::pc32:
        if constexpr (!f64) return dispatch_ncb<1, 8>(l.ncb, [&](auto NCB) {
            static_assert(jtj_pc32_lds_bytes(NCB) == JtjPc32Cfg<NCB>::LDS_BYTES, "jtj_plan.h: k_jtj_pc32 LDS size");
            return launch_one<k_jtj_pc32<NCB>>(l, JtjPc32Cfg<NCB>::THREADS, s, a);
        });
        break;
    case JtjKernel::ring8:
        if constexpr (f64) return dispatch_ncb<9, 16>(l.ncb, [&](auto NCB) {
            static_assert(jtj8_lds_bytes(NCB) == Jtj8Cfg<NCB>::LDS_BYTES, "jtj_plan.h: k_jtj8 LDS size");
            return launch_one<k_jtj8<NCB>>(l, kJtj8Threads, s, a, rewrite ? 1 : 0);
        });
        break;
    case JtjKernel::fdp8:                                  // compiled for n rounded up to a multiple of 32; DIFF: of 64
        if constexpr (f64) {
            if (diff) return dispatch_ncb<12, 16, 4>(l.ncb, [&](auto NCB) { return fdp8_one<NCB, true, false>(l, a, s); });
            return dispatch_ncb<10, 16, 2>(l.ncb, [&](auto NCB) {
                return op == JtjOp::plain ? fdp8_one<NCB, false, true>(l, a, s) : fdp8_one<NCB, false, false>(l, a, s);
            });
        }
        break;
    case JtjKernel::wide: {                                // the Broyden rewrite is a separate pass in front
        if (rewrite) {
            const size_t G = (a.m + 3) / 4;
            size_t blocks = (G + 3) / 4;
            if (blocks > 2048) blocks = 2048;
            if (a.n <= 256)
                MIRLSQ_LAUNCH(k_broyden_wide<T>, dim3((unsigned)blocks), dim3(256), 0, s, a.Jout, a.y, a.y_old, a.dx, a.dx_dot, a.m, a.n);
            else
                MIRLSQ_LAUNCH(k_broyden_rows<T>, dim3((unsigned)blocks), dim3(256), 0, s, a.Jout, a.y, a.y_old, a.dx, a.dx_dot, a.m, a.n);
        }
        JtjWideArgs<T> w{};
        w.J = a.J; w.y = a.y; w.slabs = a.slabs; w.m = a.m; w.n = a.n;
        w.nt = (l.ncb + kWideTile - 1) / kWideTile;
        return launch_one<k_jtj_wide<T>>(l, 256, s, w);
    }
    case JtjKernel::none: break;
    }
    return hipErrorInvalidValue;
}

}  // namespace

template <typename T>
hipError_t jtj_run(const JtjPlan& p, JtjOp op, const JtjArgs<T>& a, T* packed, hipStream_t s, const JtjUnpack<T>& u)
{
    // the difference panel: fd_diff writes J, fd_diff_keep does not -- the operation says it, not the pointer
    if ((op == JtjOp::fd_diff || op == JtjOp::fd_diff_keep) && (op == JtjOp::fd_diff_keep) != (a.Jout == nullptr)) return hipErrorInvalidValue;
    const JtjLaunch l = jtj_resolve(p, op, reinterpret_cast<uintptr_t>(a.J) % 16 == 0);
    const hipError_t e = launch_kernel<T>(l, op, a, s);
    if (e != hipSuccess) return e;
    if (l.kernel == JtjKernel::wide)   // per tile pair; every one-job kernel: the shared slab reduction -> packed[ n(n+1)/2 + n ] (+ u)
        MIRLSQ_LAUNCH(k_jtj_wide_reduce<T>, dim3((kWideSlabLen + 31) / 32, l.njobs), dim3(256), 0, s, a.slabs, l.nblk, a.n, packed);
    else
        MIRLSQ_LAUNCH(k_jtj_slab_reduce<T>, dim3((l.slab_len + 31) / 32), dim3(1024), 0, s, a.slabs, l.nblk, l.slab_len, l.ncb, a.n, packed, u.JJ, u.Jy);
    return hipGetLastError();
}

template <typename T>
hipError_t jtj_unpack(const T* packed, int n, T* JJ, T* Jy, LmState<T>* st, hipStream_t s)
{
    MIRLSQ_LAUNCH(k_unpack_grad<T>, dim3(n + 1), dim3(128), 0, s, packed, n, JJ, Jy, st);
    return hipGetLastError();
}

#define MIRLSQ_INSTANTIATE(T)                                                                                                              \
    template hipError_t jtj_run<T>(const JtjPlan&, JtjOp, const JtjArgs<T>&, T*, hipStream_t, const JtjUnpack<T>&);                        \
    template hipError_t jtj_unpack<T>(const T*, int, T*, T*, LmState<T>*, hipStream_t);
MIRLSQ_INSTANTIATE(double)
MIRLSQ_INSTANTIATE(float)
#undef MIRLSQ_INSTANTIATE

}  // namespace mirlsq

MIRLSQ_DEFINE_PRELOAD(jtj)
