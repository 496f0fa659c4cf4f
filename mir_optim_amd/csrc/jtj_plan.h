// jtj_plan.h -- host view of the J^T J kernels: their argument block, which kernel runs for a shape and an operation
// (jtj_plan<T>(), the ONE place that decides it) and the launch entry point (defined in launch_jtj.hip, the only translation
// unit that instantiates the kernels). LS = source/mir/optim/least_squares.d of the reference.
//
// Operations (JtjOp): plain = J^T J + J^T y of a given J (LS:1052, 1065); rewrite = the same behind the Broyden update as the
// literal restatement of LS:1003-1006, J rewritten (MIR_LSQ_VARIANT_BROYDEN_REWRITE); fd = finite-difference pair panel -> J,
// J^T J, J^T y (LS:1041-1047 fused); fd_diff = the same from the difference panel; fd_diff_keep = the difference panel -> J^T J,
// J^T y alone: J is not written, the caller keeps the panel itself as J0 (Jout == nullptr). Kernel by shape and operation:
//   shape                                      plain               rewrite               fd            fd_diff                   fd_diff_keep
//   f64, n <= 128                              fdp <., false> (1)  stream <., ., true>   fdp <., true> fdp <., false, true> (1)  fdp_nw (5)
//   f64, 128 < n <= 256, n % 16 == 0, m even   ring8               ring8, Broyden flag   fdp8          fdp8 <., true> (2)        as fd_diff
//   f64, 128 < n <= 256, the other n and m     fdp8 <., false, true>   wide (3)          fdp8          fdp8 <., true> (2)        as fd_diff
//   f32, n <= 128, n % 4 == 0                  pc32 (4)            stream <., ., true>   none          none                      none
//   f32, n <= 128, n % 4 != 0                  stream              stream <., ., true>   none          none                      none
//   n > 256; f32, n > 128                      wide                wide (3)              none          none                      none
// stream = k_jtj (register streaming), fdp = k_jtj_fdp, fdp_nw = k_jtj_fdp_nw (fdp's store-free instance: same grid, LDS, slabs),
// pc32 = k_jtj_pc32, ring8 = k_jtj8 (eight-wave LDS-DMA ring), fdp8 = k_jtj_fdp8 (compiled for n rounded up to a multiple of 32),
// wide = k_jtj_wide (64-column tile-pair jobs, any n).
// (1) the flat producer (8-byte aligned loads) for odd n, for the difference panel with n % 16 != 0 and -- decided at the launch,
//     jtj_resolve -- for a J that is not 16-byte aligned.  (2) n % 64 == 0 only (n = 192, 256), else none.
// (3) k_broyden_wide (n <= 256) / k_broyden_rows in front.  (4) a J that is not 16-byte aligned: stream_fallback (jtj_resolve).
// (5) where fd_diff is fdp's strided producer (n % 16 == 0) and a workgroup's rows span less than 4 GB (k_jtj_fdp_nw addresses them
//     with 32-bit byte offsets); else fd_diff's entry: fdp with a null Jout. A panel that is not 16-byte aligned: fdp's flat producer.
//
// Offset views. Only J (plain, rewrite) and the difference panel / Jout (fd_diff, fd_diff_keep) may be element-aligned views handed to a unit
// entry; y, y_old, dx, twh and the pair panel of `fd` are the library's own buffers and always 16-byte aligned. What is verified,
// at kernel level (tests/jtj_cases.py, tests/test_gpu_jtj_cells.py; tests/test_jtj_cell_coverage.py proves that every instance
// launch_jtj.hip compiles is in that list): with every buffer between NaN guard bands that must come back bit-identical, each
// instance is bit-exact on exact-integer data, inside the forward bound gamma_m |J|^T |J| on random data, deterministic, keeps a
// NaN of the last row to its row and column, and -- stream, fdp's flat producer, fdp8's plain flavour, wide and the reroutings
// of jtj_resolve -- gives the bits of the aligned run for a J one element off the 16-byte grid.
// OPEN: ring8 at an offset pointer. k_jtj8 issues 16-byte global_load_lds from J, y and y_old, jtj_resolve keeps ring8 for an
// unaligned J, and nothing in the code establishes that a 16-byte LDS-DMA from an 8-byte-aligned address is defined. It is not
// run anywhere; rerouting it (fdp8's plain flavour / wide take any pointer) is the follow-up.
#pragma once

#include <initializer_list>

#include "../../include/mir_optim_amd.h"
#include "common.h"

namespace mirlsq {

template <typename T>
struct JtjArgs {
    const T* J;        // m x n row-major
    T* Jout;           // BROYDEN: where updated rows are written (== J for in-place)
    const T* y;        // residual at the current point (length m)
    const T* y_old;    // BROYDEN: residual at the previous point (the reference's mBuffer after swap, LS:1136)
    const T* dx;       // BROYDEN: accepted step (length n)
    const T* dx_dot;   // BROYDEN: device scalar ||dx||^2 (LS:1002: d = 1 / deltaX_dot)
    T* slabs;          // gridDim.x slabs of jtj_slab_len<NCB>() elements
    size_t m;
    int n;
    const T* twh;      // finite-difference kernels (jtj_fdp.h, jtj_fdp8.h): interval widths xph - xmh (LS:1031); then J is the
                       // m x 2n row-major panel of perturbed residuals [f(x + h e_j), f(x - h e_j)]_j and Jout receives the Jacobian
};

constexpr int kJtjWaves = 4;   // waves per workgroup

template <int NCB> __host__ __device__ constexpr int jtj_nacc() { return NCB * (NCB + 1) / 2; }
// slab: NACC blocks x 4 registers x 64 lanes, then NCB x 64 lanes of J^T y partials
template <int NCB> __host__ __device__ constexpr int jtj_slab_len() { return (jtj_nacc<NCB>() * 4 + NCB) * kWave; }
// The accumulator blocks are split over 1, 2 or 4 "roles" (waves that walk the same rows) so that
// one wave keeps at most 96 accumulator VGPRs (regs_per_block = 4 for f32, 8 for f64).
__host__ __device__ constexpr int jtj_roles_rt(int ncb, int regs_per_block)
{
    const int regs = ncb * (ncb + 1) / 2 * regs_per_block;
    return regs <= 96 ? 1 : (regs <= 192 ? 2 : 4);
}

// tile-pair jobs (jtj_wide.h)
constexpr int kWideTile = 4;                                             // blocks per tile side
constexpr int kWideSlabLen = (kWideTile * kWideTile * 4 + kWideTile) * kWave;   // 16 blocks x 4 regs + 4 jy regs, x 64 lanes
// dynamic LDS of the kernels that size it at compile time (launch_jtj.hip asserts the match with the kernels' Cfg structs)
constexpr size_t jtj8_lds_bytes(int ncb) { return (size_t)4 * 16 * 16 * ncb * 8 + 2 * 4 * 1024; }   // four 16-row stages + the y / y_old rings
constexpr size_t jtj_fdp_lds_bytes(int ncb, bool fd) { return (size_t)2 * (fd && ncb % 4 ? 16 : 32) * (16 * ncb + 1) * 8; }   // two stages of 16 / 32 rows + y
constexpr int kJtjFdpStageRows = 32;                                                                // JtjFdpCfg<NCB, false>::RS
constexpr size_t jtj_fdp_flat_bytes(int ncb) { return (size_t)16 * ncb * 8; }                       // + the 1 / twh table of the flat producer
constexpr size_t jtj_fdp8_lds_bytes(int ncb) { return (size_t)2 * 16 * (16 * ncb + 17) * 8; }
constexpr size_t jtj_pc32_lds_bytes(int ncb) { return (size_t)2 * 64 * (16 * ncb + 17) * 4; }

// Where the slab reduction may put its result besides `packed`: the full symmetric J^T J and J^T y (the work of
// k_unpack_grad; max |J^T y| is taken by the solve kernel), when no all-reduce of `packed` sits in between. All null: `packed` only.
template <typename T>
struct JtjUnpack {
    T* JJ = nullptr; T* Jy = nullptr;
};

enum class JtjKernel { none, stream, fdp, pc32, ring8, fdp8, wide, fdp_nw };   // none: the shape is not covered for this operation
enum class JtjOp { plain, rewrite, fd, fd_diff, fd_diff_keep };
struct JtjLaunch {
    JtjKernel kernel = JtjKernel::none;
    int ncb = 0;        // 16-column blocks the kernel is compiled for = the layout of its slabs (fdp8: even, >= ceil(n / 16)); wide: ceil(n / 16)
    int nblk = 0;       // grid.x = slabs per job
    int njobs = 1;      // grid.y (wide: tile pairs)
    int slab_len = 0;
    size_t lds = 0;     // dynamic LDS
    bool flat = false;  // fdp: the flat producer
};
struct JtjPlan {
    JtjLaunch plain, rewrite, fd, fd_diff, fd_diff_keep;
    JtjLaunch stream_fallback;      // what `plain` becomes when J is not 16-byte aligned (pc32 only; else none)
    const JtjLaunch& of(JtjOp op) const
    {
        const JtjLaunch* const e[] = {&plain, &rewrite, &fd, &fd_diff, &fd_diff_keep};
        return *e[(int)op];
    }
};

template <typename T>
JtjPlan jtj_plan(size_t m, int n, int num_cu)
{
    constexpr bool f64 = sizeof(T) == 8;
    using K = JtjKernel;
    const int ncb = (n + 15) / 16;
    auto slab_len = [](int c) { return (c * (c + 1) / 2 * 4 + c) * kWave; };
    // grid: about 8 (`per`) units of `unit` rows a workgroup, at least one workgroup, at most `cap`
    auto grid = [m](size_t unit, size_t per, size_t cap) {
        const size_t want = ((m + unit - 1) / unit + per - 1) / per;
        return (int)(want < cap ? (want ? want : 1) : cap);
    };
    auto wide = [&] {           // any n: 64-column tile pairs; at least ~8 four-row groups per wave, four workgroups per CU over all jobs
        const int nt = (ncb + kWideTile - 1) / kWideTile, njobs = nt * (nt + 1) / 2;
        const size_t cap = (size_t)num_cu * 4 / njobs;
        return JtjLaunch{K::wide, ncb, grid(4, 4 * 8, cap < 1 ? 1 : cap), njobs, kWideSlabLen, (size_t)2 * kWideSlabLen * sizeof(T)};
    };
    JtjPlan p;
    if (n > 256 || (!f64 && n > 128)) {
        p.plain = p.rewrite = wide();
        return p;
    }
    if (n > 128) {
        // fdp8, any n: compiled for an even number of blocks; ring8 and fdp8: 16-row stages, at least ~8 a workgroup, one workgroup per CU
        const int ncb8 = 2 * ((n + 31) / 32), nblk = grid(16, 8, (size_t)num_cu);
        p.fd = {K::fdp8, ncb8, nblk, 1, slab_len(ncb8), jtj_fdp8_lds_bytes(ncb8)};
        if (n % 64 == 0) p.fd_diff = p.fd_diff_keep = p.fd;      // two columns per 16-byte load: whole loads per row
        if (n % 16 == 0 && m % 2 == 0) p.plain = p.rewrite = {K::ring8, ncb, nblk, 1, slab_len(ncb), jtj8_lds_bytes(ncb)};
        else { p.plain = p.fd; p.rewrite = wide(); }
        return p;
    }
    {
        const int rpb = 4 * (int)(sizeof(T) / 4), nacc = ncb * (ncb + 1) / 2;
        const int roles = jtj_roles_rt(ncb, rpb);
        const size_t lds = (size_t)(roles == 4 ? 0 : (roles == 2 ? 1 : 2)) * slab_len(ncb) * sizeof(T);
        // workgroups per CU: LDS- and register-limited (one workgroup = one wave per SIMD)
        int per_cu = lds ? (int)((160 * 1024) / lds) : 8;
        const int reg_waves = (nacc * rpb / roles > 40) ? 2 : 4;   // matches jtj_min_waves
        if (per_cu > reg_waves) per_cu = reg_waves;
        if (per_cu < 1) per_cu = 1;
        // at least ~8 four-row groups per wave
        p.rewrite = {K::stream, ncb, grid(4, (size_t)(kJtjWaves / roles) * 8, (size_t)num_cu * per_cu), 1, slab_len(ncb), lds};
    }
    if (f64) {
        p.fd = {K::fdp, ncb, p.rewrite.nblk, 1, slab_len(ncb), jtj_fdp_lds_bytes(ncb, true)};   // on k_jtj's grid, except:
        if (n % 16 == 0 && m % 2 == 0) {
            // the shapes k_jtj_fdp was tuned on: two workgroups per CU, at least ~8 blocks of rs rows each (the partition of the
            // retired LDS-DMA ring kernel; kept: it fixes the summation order of the slabs)
            const int rs = ncb <= 4 ? 32 : (ncb == 5 ? 24 : (ncb == 6 ? 20 : 16));
            p.fd.nblk = grid(rs, 8, (size_t)num_cu * 2);
        }
        p.plain = p.fd;
        p.plain.lds = jtj_fdp_lds_bytes(ncb, false);
        p.fd_diff = p.plain;
        // rows not on 16-byte boundaries; the difference panel also when a row of J does not start on a 128-byte boundary: the
        // flat producer writes J back in memory order instead of the consumers' row segments. (On the 128-byte grid the consumers'
        // write-back is the faster one: 0.428 against 0.448 ms at m = 1e6, n = 128; 0.189 against 0.196 at n = 64.)
        p.plain.flat = n % 2 != 0;
        p.fd_diff.flat = n % 16 != 0;
        for (JtjLaunch* l : {&p.plain, &p.fd_diff}) if (l->flat) l->lds += jtj_fdp_flat_bytes(ncb);
        // the store-free instance addresses a workgroup's rows (`per` stages of kJtjFdpStageRows) with 32-bit byte offsets
        p.fd_diff_keep = p.fd_diff;
        const size_t stages = (m + kJtjFdpStageRows - 1) / kJtjFdpStageRows, per = (stages + p.fd_diff.nblk - 1) / p.fd_diff.nblk;
        if (!p.fd_diff.flat && per * kJtjFdpStageRows * (size_t)n * sizeof(double) < (size_t{1} << 32)) p.fd_diff_keep.kernel = K::fdp_nw;
    } else if (n % 4 == 0) {
        // 64-row stages, at least ~4 a workgroup, two workgroups per CU
        p.plain = {K::pc32, ncb, grid(64, 4, (size_t)num_cu * 2), 1, slab_len(ncb), jtj_pc32_lds_bytes(ncb)};
        p.stream_fallback = p.rewrite;
    } else {
        p.plain = p.rewrite;
    }
    return p;
}

// The two choices that depend on the POINTER, made at the launch: k_jtj_pc32 reads J with 16-byte loads of four floats and
// k_jtj_fdp's strided producer with 16-byte loads of two doubles; a J that is not 16-byte aligned (an offset view handed to a
// unit entry) takes the register-streaming kernel / the flat producer (the pair panel of `fd` is the library's own buffer);
// so does the store-free instance, whose lean producer loads 16 bytes too.
inline JtjLaunch jtj_resolve(const JtjPlan& p, JtjOp op, bool aligned16)
{
    JtjLaunch l = p.of(op);
    if (aligned16) return l;
    if (l.kernel == JtjKernel::pc32) return p.stream_fallback;
    if (l.kernel == JtjKernel::fdp_nw) l.kernel = JtjKernel::fdp;      // the lean producer's 16-byte loads: the flat one, as fd_diff
    if (l.kernel == JtjKernel::fdp && op != JtjOp::fd && !l.flat) { l.flat = true; l.lds += jtj_fdp_flat_bytes(l.ncb); }
    return l;
}

// slab elements the J^T J kernels of a plan may write
inline size_t jtj_slab_elems(const JtjPlan& p)
{
    size_t e = 0;
    for (const JtjLaunch* l : {&p.plain, &p.rewrite, &p.fd, &p.fd_diff, &p.fd_diff_keep, &p.stream_fallback}) {
        const size_t el = (size_t)l->nblk * l->njobs * l->slab_len;
        e = e > el ? e : el;
    }
    return e;
}

// does jtj_run honour a JtjUnpack for this operation? (the tile-pair jobs have a reduction of their own)
inline bool jtj_unpacks(const JtjPlan& p, JtjOp op) { return p.of(op).kernel != JtjKernel::wide; }

// ---- launch entry points (launch_jtj.hip; instantiated for double and float). Every kernel they launch is counted in
//      tl_launches. `packed` receives [J^T J lower | J^T y]; `u` additionally the unpacked form (see JtjUnpack).
// the operation `op` on a.J -- plain / rewrite: J; fd: the m x 2n row-major pair panel, fd_diff / fd_diff_keep: the m x n difference
// panel D_ij = f(x + h e_j)_i - f(x - h e_j)_i (all with a.twh; a.Jout receives J -- fd_diff_keep: a.Jout == nullptr, and only then).
// hipErrorInvalidValue: the shape is not covered, or a.Jout does not fit the operation.
template <typename T>
hipError_t jtj_run(const JtjPlan& p, JtjOp op, const JtjArgs<T>& a, T* packed, hipStream_t s, const JtjUnpack<T>& u = {});
// packed [J^T J lower | J^T y] -> full symmetric JJ, Jy, st->jy_inf (behind a communicator's all-reduce)
template <typename T> struct LmState;
template <typename T>
hipError_t jtj_unpack(const T* packed, int n, T* JJ, T* Jy, LmState<T>* st, hipStream_t s);

}  // namespace mirlsq
