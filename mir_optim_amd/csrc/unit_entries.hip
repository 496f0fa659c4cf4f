// unit_entries.hip -- unit-level access to the kernels of the path (parity tests, micro-benchmarks) and the standalone
// BOXCQP entry: mir_solve_box_qp_gpu_* (boxcqp.d:85-102 is D-only), mir_lsq_jtj_*, mir_lsq_fd_jtj_d, mir_lsq_fd_diff_jtj_d,
// mir_lsq_lm_solve_* (one launch of the LM solve kernels; mir_lsq_lm_solve_class is host code), mir_lsq_lr_pass_* / mir_lsq_lr_flush_*
// (the read-only Broyden sweep's launches; mir_lsq_lr_class and mir_lsq_lr_blocks are host code), mir_lsq_decide_* / mir_lsq_fd_points_* /
// mir_lsq_fd_fill_* / mir_lsq_entry_state_* / mir_lsq_unpack_grad_* (the decision and bookkeeping kernels of misc_kernels.h, one launch
// each between guard bands; mir_lsq_sumsq_blocks is host code), mir_lsq_selftest_reductions, mir_fit_spline_gpu_eval_* / _eval_host_* / _factor_* (fit_spline_gpu.hip). Each call owns its scratch and synchronises before it returns. mir_lsq_jtj_plan is host code.
#include <cstddef>
#include <cstring>
#include <memory>
#include <vector>

#include "broyden_launch.h"
#include "driver.h"
#include "fit_spline_gpu.h"
#include "misc_kernels.h"

using namespace mirlsq;

namespace {
// Self-test of the wave reductions (mir_lsq_selftest_reductions): every wave_sum / wave_max of common.h against the plain
// butterfly on __shfl_xor (16, 32 last: the order whose pairs the DPP forms reproduce), bit for bit, on `rounds` pseudo-random
// inputs a lane. out[0..3] += mismatching lanes of sum<float>, sum<double>, max<float>, max<double>.
__global__ __launch_bounds__(256) void k_selftest_reductions(int rounds, uint32_t seed, int* out)
{
    // no contraction here: the multiplication that makes an input would be fused into the FIRST addition of whichever form
    // consumes it (one rounding less on one operand of one form), and the two forms would differ by construction
#pragma clang fp contract(off)
    uint32_t sr = seed ^ (0x9E3779B9u * (blockIdx.x * blockDim.x + threadIdx.x + 1));
    auto rnd = [&]() { sr ^= sr << 13; sr ^= sr >> 17; sr ^= sr << 5; return sr; };
    int bad[4] = {0, 0, 0, 0};
    for (int it = 0; it < rounds; ++it) {
        const float f = (float)(int32_t)rnd() * (1.0f / 65536.0f) * ((it & 7) == 0 ? 1e-20f : 1.0f);
        const double d = ((double)(int32_t)rnd() + (double)rnd() * 2.3283064365386963e-10) * ((it & 3) == 0 ? 1e-200 : 1.0);
        auto ref_sum = [](auto v) {
            v += __shfl_xor(v, 8, kWave); v += __shfl_xor(v, 4, kWave); v += __shfl_xor(v, 2, kWave); v += __shfl_xor(v, 1, kWave);
            v += __shfl_xor(v, 16, kWave); v += __shfl_xor(v, 32, kWave);
            return v;
        };
        auto ref_max = [](auto v) {
            for (int m : {8, 4, 2, 1, 16, 32}) { const auto o = __shfl_xor(v, m, kWave); v = o > v ? o : v; }
            return v;
        };
        const float sf = wave_sum(f), rf = ref_sum(f);
        const double sd = wave_sum(d), rdd = ref_sum(d);
        bad[0] += __float_as_uint(sf) != __float_as_uint(rf);
        bad[1] += __double_as_longlong(sd) != __double_as_longlong(rdd);
        bad[2] += __float_as_uint(wave_max(f)) != __float_as_uint(ref_max(f));
        bad[3] += __double_as_longlong(wave_max(d)) != __double_as_longlong(ref_max(d));
    }
    for (int k = 0; k < 4; ++k) if (bad[k]) atomicAdd(out + k, bad[k]);
}

template <typename T, typename QS>
int box_qp_entry(const QS* settings, size_t n_, const T* P, const T* q, const T* l, const T* u, T* x,
                 int unconstrainedSolution, int* iterations)
{
    if (iterations) *iterations = 0;
    if (n_ == 0) return mir_box_qp_solved;
    if (!device_available()) return mir_box_qp_numericError;
    const int n = (int)n_;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t oP = take(sizeof(T) * n * n), oq = take(sizeof(T) * n), ol = take(sizeof(T) * n), ou = take(sizeof(T) * n),
                 ox = take(sizeof(T) * n), oPm = take(sizeof(T) * n * n), oA = take(sizeof(T) * n * n),
                 oF = take(sizeof(T) * n * (n | 1)), ov = take(sizeof(T) * 12 * n), oi = take(sizeof(int32_t) * 2 * n),
                 oo = take(sizeof(int) * 4);
    char* base = nullptr;
    if (hipMalloc((void**)&base, off) != hipSuccess) return mir_box_qp_numericError;
    BoxQpArgs<T> a{};
    a.P = (T*)(base + oP); a.q = (T*)(base + oq); a.l = (T*)(base + ol); a.u = (T*)(base + ou); a.x = (T*)(base + ox);
    a.sc.Pm = (T*)(base + oPm); a.sc.A = (T*)(base + oA); a.sc.Fg = (T*)(base + oF); a.sc.vec = (T*)(base + ov);
    a.sc.ivec = (int32_t*)(base + oi); a.out = (int*)(base + oo); a.sc.dbg = nullptr;
    a.relTol = settings->relTolerance; a.absTol = settings->absTolerance; a.maxIterations = settings->maxIterations;
    a.unconstrained = unconstrainedSolution; a.n = n;
    a.f_in_lds = solve_nb(n, (int)sizeof(T)) > 0;
    int out[2] = {mir_box_qp_numericError, 0};
    bool good = hipMemcpy((void*)a.P, P, sizeof(T) * n * n, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy((void*)a.q, q, sizeof(T) * n, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy((void*)a.l, l, sizeof(T) * n, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy((void*)a.u, u, sizeof(T) * n, hipMemcpyHostToDevice) == hipSuccess
        && hipMemcpy((void*)a.x, x, sizeof(T) * n, hipMemcpyHostToDevice) == hipSuccess;
    if (good) good = launch_box_qp<T>(a, nullptr) == hipSuccess;
    if (good) {
        good = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess
            && hipMemcpy(out, a.out, sizeof(out), hipMemcpyDeviceToHost) == hipSuccess
            && hipMemcpy(x, a.x, sizeof(T) * n, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(base);
    if (!good) return mir_box_qp_numericError;
    if (iterations) *iterations = out[1];
    return out[0];
}

// The allocation of the entries below: regions between guard bands -- at least kLmGuardBytes of 0xFF bytes (a NaN in both types)
// in front of each region and behind the last, regions 256-byte aligned as the workspace's; band b starts at the last byte of
// region b - 1 and ends where region b starts -- everything preset to 0xFF (a read of scratch nobody wrote shows as a NaN).
// Device memory, or -- pinned -- device-mapped coherent host memory as the solver's mirror (workspace.hip).
constexpr size_t kLmGuardBytes = 4096;
struct Banded {
    struct Region { size_t off, bytes; };
    std::vector<Region> reg;
    size_t off = 0, total = 0;
    bool pinned = false;
    char* base = nullptr;        // the address the kernels are given
    char* host = nullptr;        // pinned: the host's address of the same memory
    std::unique_ptr<unsigned char[]> img;
    ~Banded() { if (pinned) { if (host) (void)hipHostFree(host); } else if (base) (void)hipFree(base); }
    size_t take(size_t count, size_t elem)
    {
        off = align_up(off + kLmGuardBytes, 256);
        reg.push_back({off, count * elem});
        off += count * elem;
        return reg.size() - 1;
    }
    bool alloc(bool pinned_ = false)
    {
        pinned = pinned_;
        total = align_up(off + kLmGuardBytes, 256);
        if (pinned) {
            if (hipHostMalloc((void**)&host, total, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { host = nullptr; return false; }
            std::memset(host, 0xFF, total);
            return hipHostGetDevicePointer((void**)&base, host, 0) == hipSuccess;
        }
        if (hipMalloc((void**)&base, total) != hipSuccess) { base = nullptr; return false; }
        return hipMemset(base, 0xFF, total) == hipSuccess;
    }
    char* at(size_t r) const { return base + reg[r].off; }
    bool up(size_t r, const void* src) const
    {
        if (!reg[r].bytes) return true;
        if (pinned) { std::memcpy(host + reg[r].off, src, reg[r].bytes); return true; }
        return hipMemcpy(at(r), src, reg[r].bytes, hipMemcpyHostToDevice) == hipSuccess;
    }
    bool zero(size_t r) const { return !reg[r].bytes || hipMemset(at(r), 0, reg[r].bytes) == hipSuccess; }   // (device memory)
    void band(size_t b, size_t& lo, size_t& hi) const { lo = b ? reg[b - 1].off + reg[b - 1].bytes : 0; hi = b < reg.size() ? reg[b].off : total; }
    // the host image, behind a device synchronisation. payload < regions: everything up to region `payload` in one copy, behind
    // it the bands alone (scratch nobody reads on the host)
    bool fetch(size_t payload = (size_t)-1)
    {
        img.reset(new unsigned char[total]);
        if (pinned) { std::memcpy(img.get(), host, total); return true; }
        if (payload >= reg.size()) return hipMemcpy(img.get(), base, total, hipMemcpyDeviceToHost) == hipSuccess;
        bool good = hipMemcpy(img.get(), base, reg[payload].off, hipMemcpyDeviceToHost) == hipSuccess;
        for (size_t b = payload + 1; b <= reg.size() && good; ++b) {
            size_t lo, hi;
            band(b, lo, hi);
            good = hipMemcpy(img.get() + lo, base + lo, hi - lo, hipMemcpyDeviceToHost) == hipSuccess;
        }
        return good;
    }
    int damaged() const          // the first band that is not intact, or -1
    {
        for (size_t b = 0; b <= reg.size(); ++b) {
            size_t lo, hi;
            band(b, lo, hi);
            for (size_t i = lo; i < hi; ++i)
                if (img[i] != 0xFF) return (int)b;
        }
        return -1;
    }
    int bands() const { return (int)reg.size() + 1; }
    const unsigned char* image(size_t r) const { return img.get() + reg[r].off; }
    void down(size_t r, void* dst) const { if (reg[r].bytes) std::memcpy(dst, image(r), reg[r].bytes); }
};
inline bool launches_done() { return hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess; }

// mir_lsq_lm_solve_*: ONE launch_lm_solve (one round's n x n part, ks ladder entries) on operands of the caller's, every device
// region the kernels are handed -- the five inputs, dx, trial, rec, the state, and each ladder entry's Pm, A, Fg, vec, ivec, coop,
// cS, at workspace.hip's sizes -- in one Banded allocation. The scratch regions start as its 0xFF pattern, the helpers' sync words
// as zero with epoch 1 (a fresh workspace's first solve), dx / trial as MIR_LSQ_LM_SOLVE_SENTINEL.
template <typename T, typename S, typename R>
int lm_solve_entry(const S* settings, size_t n_, T* JJ, T* Jy, T* x, T* lower, T* upper, int ks, const T* lam, T state_lambda,
                   unsigned mode, R* rec, T* dx, T* trial, T* jy_inf, int info[6])
{
    if (!settings || !JJ || !Jy || !x || !lower || !upper || !lam || !rec || !dx || !trial || !jy_inf || !info) return -1;
    if (n_ == 0 || n_ > 4096 || ks < 1 || ks > kChainMax || (mode & ~31u)) return -1;
    if (!device_available()) return -2;
    const int n = (int)n_;
    const size_t nn = (size_t)n * n;
    Banded d;
    const size_t rJJ = d.take(nn, sizeof(T)), rJy = d.take(n, sizeof(T)), rx = d.take(n, sizeof(T)), rlo = d.take(n, sizeof(T)),
                 rup = d.take(n, sizeof(T)), rdx = d.take((size_t)kChainMax * n, sizeof(T)), rtr = d.take((size_t)kChainMax * n, sizeof(T)),
                 rrec = d.take(kChainMax, sizeof(ChainRec<T>)), rst = d.take(1, sizeof(LmState<T>));
    size_t rsc[kChainMax][7];
    for (int k = 0; k < kChainMax; ++k) {
        rsc[k][0] = d.take(nn, sizeof(T)); rsc[k][1] = d.take(nn, sizeof(T)); rsc[k][2] = d.take((size_t)n * (n | 1), sizeof(T));
        rsc[k][3] = d.take((size_t)12 * n, sizeof(T)); rsc[k][4] = d.take((size_t)2 * n, sizeof(int32_t));
        rsc[k][5] = d.take(n > kSolveMaxN ? kCoopWords : 0, sizeof(unsigned long long));
        rsc[k][6] = d.take(coop_scratch_elems(n), sizeof(T));
    }
    if (!d.alloc()) return -3;
    LmSolveArgs<T> a{};
    a.JJ = (T*)d.at(rJJ); a.Jy = (T*)d.at(rJy); a.x = (T*)d.at(rx); a.lower = (T*)d.at(rlo); a.upper = (T*)d.at(rup);
    a.dx = (T*)d.at(rdx); a.trial = (T*)d.at(rtr); a.rec = (ChainRec<T>*)d.at(rrec); a.st = (LmState<T>*)d.at(rst);
    a.set = lm_settings_dev(settings); a.n = n;
    for (int k = 0; k < kChainMax; ++k) {
        a.sc[k].Pm = (T*)d.at(rsc[k][0]); a.sc[k].A = (T*)d.at(rsc[k][1]); a.sc[k].Fg = (T*)d.at(rsc[k][2]); a.sc[k].vec = (T*)d.at(rsc[k][3]);
        a.sc[k].ivec = (int32_t*)d.at(rsc[k][4]); a.sc[k].dbg = nullptr; a.sc[k].coop = (unsigned long long*)d.at(rsc[k][5]);
        a.sc[k].cS = (T*)d.at(rsc[k][6]);
        a.lam[k] = k < ks ? lam[k] : T(0);
    }
    a.f_in_lds = solve_nb(n, (int)sizeof(T)) > 0;
    a.check_grad = (mode & 1u) ? 1 : 0;
    a.lambda_from_state = (mode & 2u) ? 1 : 0;
    bool bounded = (mode & 4u) != 0;
    for (int i = 0; i < n; ++i)
        if (lower[i] > -Lim<T>::inf() || upper[i] < Lim<T>::inf()) bounded = true;
    const bool generic = (mode & 8u) != 0;
    a.coop_w = coop_width(n, query_num_cu(), !(mode & 16u));
    a.coop_epoch = a.coop_w > 1 ? 1u : 0u;
    const LmSolveClass cls = lm_solve_class((int)sizeof(T), n, bounded, generic, false);
    info[0] = cls.kind; info[1] = cls.nb; info[2] = cls.bounded; info[3] = a.coop_w; info[4] = -1; info[5] = d.bands();

    LmState<T> st{};
    st.lambda = state_lambda;
    std::vector<T> sentinel((size_t)kChainMax * n, T(MIR_LSQ_LM_SOLVE_SENTINEL));
    bool good = d.up(rJJ, JJ) && d.up(rJy, Jy) && d.up(rx, x) && d.up(rlo, lower) && d.up(rup, upper) && d.up(rdx, sentinel.data())
        && d.up(rtr, sentinel.data()) && d.up(rst, &st);
    for (int k = 0; k < kChainMax; ++k) good = good && d.zero(rsc[k][5]);
    if (!good) return -3;
    if (launch_lm_solve<T>(a, ks, bounded, generic, nullptr) != hipSuccess) { (void)hipDeviceSynchronize(); return -4; }
    // the scratch is 3 n^2 elements a ladder entry and nobody reads it here: the payloads in front of it, behind them the bands
    if (!launches_done() || !d.fetch(rsc[0][0])) return -5;
    info[4] = d.damaged();
    d.down(rJJ, JJ); d.down(rJy, Jy); d.down(rx, x); d.down(rlo, lower); d.down(rup, upper); d.down(rdx, dx); d.down(rtr, trial);
    std::vector<ChainRec<T>> rh(kChainMax);
    d.down(rrec, rh.data());
    for (int k = 0; k < ks; ++k) {
        rec[k].lambda = rh[k].lambda; rec[k].new_dx_dot = rh[k].new_dx_dot; rec[k].predicted = rh[k].predicted;
        rec[k].trial_xnorm = rh[k].trial_xnorm; rec[k].qp_status = rh[k].qp_status; rec[k].qp_iterations = rh[k].qp_iterations;
        rec[k].flags = rh[k].flags; rec[k].reserved = 0;
    }
    d.down(rst, &st);
    *jy_inf = st.jy_inf;
    return 0;
}

// mir_lsq_lr_pass_*: the launches of Solver::broyden_lowrank behind its flush, without a communicator -- lr_sweep, lr_reduce,
// lr_finish (not in speculation mode: the fused round's n x n side lives in the solve kernel) on the solver's lr_blocks(m, num_cu)
// workgroups -- and then lr_sumsq + lr_sumsq_final over `count` m-vectors at y (vector 0 is the sweep's y). J, U, D, dx, dx_dot, y,
// y_old, JJ, Jy are DEVICE pointers of the caller's; what the solver keeps in its workspace -- the partials, the reduced vector,
// the stage-1 partials of the sums (pstride = the workgroup count, so that the region ends with the last partial), the sums, the
// state and the record -- lies in one Banded allocation of the call's.
template <typename T, typename R>
int lr_pass_entry(size_t m, size_t n_, int k, const T* J, const T* twh, T* U, T* D, const T* dx, const T* dx_dot, const T* y, int count,
                  const T* y_old, T* JJ, T* Jy, const R* spec, T absTolerance, T relTolerance, T* partials, T* reduced, T* sums,
                  T* jy_inf, int info[6])
{
    if (!J || !U || !D || !dx || !dx_dot || !y || !y_old || !JJ || !Jy || !partials || !reduced || !sums || !jy_inf || !info) return -1;
    if (m == 0 || n_ == 0 || n_ > (size_t)kLrMaxN || k < 0 || k >= kLrMax || count < 1 || count > kChainMax) return -1;
    if (!device_available()) return -2;
    const int n = (int)n_, len = lr_len(n), nblk = lr_blocks(m, query_num_cu());
    Banded d;
    const size_t rpart = d.take((size_t)nblk * len, sizeof(T)), rvec = d.take(len, sizeof(T)), rsp = d.take((size_t)count * nblk, sizeof(T)),
                 rsum = d.take(count, sizeof(T)), rst = d.take(1, sizeof(LmState<T>)), rrec = d.take(1, sizeof(ChainRec<T>));
    if (!d.alloc()) return -3;
    const LrClass cls = lr_class_of<T>(n, J);
    info[0] = cls.ncp; info[1] = cls.vec; info[2] = nblk; info[3] = -1; info[4] = d.bands(); info[5] = 0;
    ChainRec<T> rec{};
    if (spec) {
        rec.lambda = spec->lambda; rec.new_dx_dot = spec->new_dx_dot; rec.predicted = spec->predicted; rec.trial_xnorm = spec->trial_xnorm;
        rec.qp_status = spec->qp_status; rec.qp_iterations = spec->qp_iterations; rec.flags = spec->flags; rec.pad = spec->reserved;
        if (!d.up(rrec, &rec)) return -3;
    }
    LrArgs<T> a{};
    a.J = J; a.U = U; a.D = D; a.dx = dx; a.dx_dot = dx_dot; a.y = y; a.y_old = y_old;
    a.partials = (T*)d.at(rpart); a.m = m; a.n = n; a.k = k;
    a.spec_rec = spec ? (const ChainRec<T>*)d.at(rrec) : nullptr;
    a.absTolerance = absTolerance; a.relTolerance = relTolerance;
    const bool good = lr_sweep<T>(a, nblk, nullptr, twh) == hipSuccess     // twh != nullptr: J is the unscaled difference panel
        && lr_reduce<T>((const T*)d.at(rpart), nblk, n, (T*)d.at(rvec), nullptr) == hipSuccess
        && (spec || lr_finish<T>((const T*)d.at(rvec), D, dx, k, n, JJ, Jy, (LmState<T>*)d.at(rst), nullptr) == hipSuccess)
        && lr_sumsq<T>(y, m, count, m, (T*)d.at(rsp), nblk, nblk, nullptr) == hipSuccess
        && lr_sumsq_final<T>((const T*)d.at(rsp), nblk, nblk, count, (T*)d.at(rsum), nullptr) == hipSuccess;
    if (!good) { (void)hipDeviceSynchronize(); return -4; }
    if (!launches_done() || !d.fetch()) return -5;
    info[3] = d.damaged();
    // the state but for jy_inf, and the record: nobody writes them (info[5]: 1 the state, 2 the record, 3 both)
    const size_t jlo = offsetof(LmState<T>, jy_inf), jhi = jlo + sizeof(T);
    for (size_t i = 0; i < sizeof(LmState<T>); ++i)
        if ((i < jlo || i >= jhi || spec) && d.image(rst)[i] != 0xFF) info[5] |= 1;
    std::vector<unsigned char> want(sizeof rec, 0xFF);
    if (spec) std::memcpy(want.data(), &rec, sizeof rec);
    if (std::memcmp(d.image(rrec), want.data(), sizeof rec) != 0) info[5] |= 2;
    d.down(rpart, partials); d.down(rvec, reduced); d.down(rsum, sums);
    std::memcpy(jy_inf, d.image(rst) + jlo, sizeof(T));
    return 0;
}

// mir_lsq_lr_flush_*: one lr_flush on device pointers of the caller's
template <typename T>
int lr_flush_entry(size_t m, size_t n, int k, T* J, const T* U, const T* D, int info[2])
{
    if (!J || !U || !D || !info || m == 0 || n == 0 || n > (size_t)kLrMaxN || k < 1 || k > kLrMax) return -1;
    if (!device_available()) return -2;
    const LrClass cls = lr_class_of<T>((int)n, J);
    info[0] = cls.ncp; info[1] = cls.vec;
    if (lr_flush<T>(J, U, D, k, m, (int)n, query_num_cu(), nullptr) != hipSuccess) { (void)hipDeviceSynchronize(); return -4; }
    return hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess ? 0 : -5;
}

template <typename T> struct StateAbi;
template <> struct StateAbi<double> { using type = mir_lsq_lm_state_d; using rec = mir_lsq_lm_solve_record_d; };
template <> struct StateAbi<float> { using type = mir_lsq_lm_state_s; using rec = mir_lsq_lm_solve_record_s; };
template <typename T> constexpr bool state_abi_ok()
{
    using A = typename StateAbi<T>::type;
    return sizeof(A) == sizeof(LmState<T>) && offsetof(A, jy_inf) == offsetof(LmState<T>, jy_inf)
        && offsetof(A, qp_status) == offsetof(LmState<T>, qp_status) && offsetof(A, iterations) == offsetof(LmState<T>, iterations)
        && offsetof(A, null_tail) == offsetof(LmState<T>, null_tail) && offsetof(A, seq) == offsetof(LmState<T>, seq)
        && offsetof(A, coop_rescued) == offsetof(LmState<T>, coop_rescued) && offsetof(A, spec_ok) == offsetof(LmState<T>, spec_ok)
        && sizeof(typename StateAbi<T>::rec) == sizeof(ChainRec<T>) && offsetof(typename StateAbi<T>::rec, flags) == offsetof(ChainRec<T>, flags);
}
static_assert(state_abi_ok<double>() && state_abi_ok<float>(), "mir_lsq_lm_state_* / mir_lsq_lm_solve_record_* are LmState / ChainRec");

// mir_lsq_decide_*: ONE k_decide_chain launch with the solver's geometry (Solver::enqueue_decide) on host operands.
template <typename T, typename S>
int decide_entry(const S* settings, size_t n_, int ks, unsigned mode, uint32_t maxIterations, uint32_t seq, void* state, void* rec,
                 T* sums, T* x, T* trial, T* dx_chain, T* dx_acc, T* partials, int nparts, int pstride, void* host_state, T* host_x,
                 int info[2])
{
    if (!settings || !state || !rec || !sums || !x || !trial || !dx_chain || !dx_acc || !host_state || !host_x || !info) return -1;
    if (n_ == 0 || n_ > (size_t)1 << 20 || ks < 1 || ks > kChainMax || (mode & ~15u)) return -1;
    if (nparts < 0 || (nparts > 0 && (!partials || pstride < nparts))) return -1;
    if (!device_available()) return -2;
    const int n = (int)n_;
    const bool mirror = (mode & MIR_LSQ_DECIDE_MIRROR) != 0;
    Banded d, p;
    const size_t rsum = d.take(ks, sizeof(T)), rrec = d.take(ks, sizeof(ChainRec<T>)), rst = d.take(1, sizeof(LmState<T>)),
                 rx = d.take(n, sizeof(T)), rtr = d.take((size_t)ks * n, sizeof(T)), rdc = d.take((size_t)ks * n, sizeof(T)),
                 rda = d.take(n, sizeof(T)), rpa = d.take(nparts > 0 ? (size_t)ks * pstride : 0, sizeof(T));
    const size_t pst = p.take(1, sizeof(LmState<T>)), px = p.take(n, sizeof(T));
    if (!d.alloc() || (mirror && !p.alloc(true))) return -3;
    bool good = d.up(rsum, sums) && d.up(rrec, rec) && d.up(rst, state) && d.up(rx, x) && d.up(rtr, trial) && d.up(rdc, dx_chain)
        && d.up(rda, dx_acc) && d.up(rpa, partials);
    if (!good) return -3;
    DecideArgs<T> a{};
    a.sums = (T*)d.at(rsum); a.rec = (const ChainRec<T>*)d.at(rrec); a.st = (LmState<T>*)d.at(rst); a.set = lm_settings_dev(settings);
    a.x = (T*)d.at(rx); a.trial = (const T*)d.at(rtr); a.dx_chain = (const T*)d.at(rdc); a.dx_acc = (T*)d.at(rda);
    a.n = n; a.ks = ks; a.check_grad = (mode & MIR_LSQ_DECIDE_CHECK_GRAD) ? 1 : 0;
    a.lambda_from_state = (mode & MIR_LSQ_DECIDE_LAMBDA_FROM_STATE) ? 1 : 0;
    a.host_st = mirror ? (LmState<T>*)p.at(pst) : nullptr; a.host_x = mirror ? (T*)p.at(px) : nullptr; a.seq = seq;
    a.spec_static = (mode & MIR_LSQ_DECIDE_SPEC_STATIC) ? 1 : 0; a.maxIterations = maxIterations;
    a.partials = (const T*)d.at(rpa); a.nparts = nparts; a.pstride = pstride;
    hipLaunchKernelGGL(k_decide_chain<T>, dim3(1), dim3(kSolveThreads), 0, nullptr, a);
    if (!launches_done() || !d.fetch() || (mirror && !p.fetch())) return -5;
    info[0] = d.damaged(); info[1] = d.bands() + (mirror ? p.bands() : 0);
    if (info[0] < 0 && mirror && p.damaged() >= 0) info[0] = d.bands() + p.damaged();
    d.down(rsum, sums); d.down(rrec, rec); d.down(rst, state); d.down(rx, x); d.down(rtr, trial); d.down(rdc, dx_chain);
    d.down(rda, dx_acc); d.down(rpa, partials);
    std::memset(host_state, 0xFF, sizeof(LmState<T>));
    std::memset(host_x, 0xFF, sizeof(T) * n);
    if (mirror) { p.down(pst, host_state); p.down(px, host_x); }
    return 0;
}

// mir_lsq_fd_points_*: ONE k_fd_points launch (64 threads; n workgroups, n + 1 with the base row) and the host's widths
template <typename T>
int fd_points_entry(size_t n_, const T* x, const T* lower, const T* upper, T eps, int with_base, T* X, T* twh, T* twh_host, int info[2])
{
    if (!x || !lower || !upper || !X || !twh || !twh_host || !info || n_ == 0 || n_ > 4096) return -1;
    if (!device_available()) return -2;
    const int n = (int)n_;
    const size_t rows = 2 * n_ + (with_base ? 1 : 0);
    Banded d;
    const size_t rx = d.take(n, sizeof(T)), rlo = d.take(n, sizeof(T)), rup = d.take(n, sizeof(T)), rX = d.take(rows * n, sizeof(T)),
                 rt = d.take(n, sizeof(T));
    if (!d.alloc() || !d.up(rx, x) || !d.up(rlo, lower) || !d.up(rup, upper)) return -3;
    hipLaunchKernelGGL(k_fd_points<T>, dim3(n + (with_base ? 1 : 0)), dim3(64), 0, nullptr, (const T*)d.at(rx), (const T*)d.at(rlo),
                       (const T*)d.at(rup), eps, n, (T*)d.at(rX), (T*)d.at(rt));
    if (!launches_done() || !d.fetch()) return -5;
    info[0] = d.damaged(); info[1] = d.bands();
    d.down(rX, X); d.down(rt, twh);
    fd_widths<T>(x, lower, upper, eps, n_, twh_host);
    return 0;
}

// mir_lsq_fd_fill_*: ONE k_fd_fill launch on the grid of Solver::fd_device, or (col) ONE k_fd_fill_col launch as Solver::fd_task's
template <typename T>
int fd_fill_entry(size_t m, size_t n_, size_t ldy, int j0, int pc, const T* Y, const T* twh, T* J, int col, int info[2])
{
    if (!Y || !twh || !J || !info || m == 0 || n_ == 0 || n_ > 4096 || m > (size_t)1 << 24 || ldy < m) return -1;
    if (j0 < 0 || pc < 1 || (size_t)j0 + pc > n_ || (col && pc != 1)) return -1;
    if (!device_available()) return -2;
    const int n = (int)n_;
    Banded d;
    // the panel ends with its last row's m-th element: a read behind it is a NaN
    const size_t ry = d.take((size_t)(2 * pc - 1) * ldy + m, sizeof(T)), rt = d.take(n, sizeof(T)), rJ = d.take(m * n_, sizeof(T));
    if (!d.alloc() || !d.up(ry, Y) || !d.up(rt, twh) || !d.up(rJ, J)) return -3;
    const T* Yd = (const T*)d.at(ry);
    if (col) {
        hipLaunchKernelGGL(k_fd_fill_col<T>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, Yd, Yd + ldy, twh[j0], (T*)d.at(rJ),
                           m, n, j0);
    } else {
        dim3 grid((unsigned)((m + 63) / 64), (unsigned)((pc + 31) / 32));
        hipLaunchKernelGGL(k_fd_fill<T>, grid, dim3(256), 0, nullptr, Yd, ldy, (const T*)d.at(rt), (T*)d.at(rJ), m, n, j0, pc);
    }
    if (!launches_done() || !d.fetch()) return -5;
    info[0] = d.damaged(); info[1] = d.bands();
    d.down(rJ, J);
    return 0;
}

// mir_lsq_entry_state_*: the launches of Solver::sumsq on sumsq_blocks(m) workgroups and k_init_state with a mirror (the entry of
// a solve, LS:953-971); then k_sumsq_partial on a grid of (nb, 2) over the two vectors at v (m apart, nb partials each) with
// k_sumsq_final on two workgroups; then k_reset_mu on the state image st2.
template <typename T>
int entry_state_entry(size_t m, const T* v, uint32_t seq, T* partials, T* sum, void* state, void* host_state, T* partials2, T* sums2,
                      void* st2, int info[3])
{
    if (!v || !partials || !sum || !state || !host_state || !partials2 || !sums2 || !st2 || !info || m == 0 || m > (size_t)1 << 28) return -1;
    if (!device_available()) return -2;
    const int nb = sumsq_blocks(m);
    Banded d, p;
    const size_t rv = d.take(2 * m, sizeof(T)), rp = d.take(nb, sizeof(T)), rs = d.take(1, sizeof(T)), rst = d.take(1, sizeof(LmState<T>)),
                 rp2 = d.take((size_t)2 * nb, sizeof(T)), rs2 = d.take(2, sizeof(T)), rst2 = d.take(1, sizeof(LmState<T>));
    const size_t pst = p.take(1, sizeof(LmState<T>));
    if (!d.alloc() || !p.alloc(true) || !d.up(rv, v) || !d.up(rst2, st2)) return -3;
    const T* vd = (const T*)d.at(rv);
    hipLaunchKernelGGL(k_sumsq_partial<T>, dim3(nb), dim3(256), 0, nullptr, vd, m, (T*)d.at(rp), (size_t)0, kPartials);
    hipLaunchKernelGGL(k_sumsq_final<T>, dim3(1), dim3(256), 0, nullptr, (const T*)d.at(rp), nb, (T*)d.at(rs), kPartials);
    hipLaunchKernelGGL(k_init_state<T>, dim3(1), dim3(1), 0, nullptr, (const T*)d.at(rs), (LmState<T>*)d.at(rst), (LmState<T>*)p.at(pst), seq);
    hipLaunchKernelGGL(k_sumsq_partial<T>, dim3(nb, 2), dim3(256), 0, nullptr, vd, m, (T*)d.at(rp2), m, nb);
    hipLaunchKernelGGL(k_sumsq_final<T>, dim3(2), dim3(256), 0, nullptr, (const T*)d.at(rp2), nb, (T*)d.at(rs2), nb);
    hipLaunchKernelGGL(k_reset_mu<T>, dim3(1), dim3(1), 0, nullptr, (LmState<T>*)d.at(rst2));
    if (!launches_done() || !d.fetch() || !p.fetch()) return -5;
    info[0] = nb; info[1] = d.damaged(); info[2] = d.bands() + p.bands();
    if (info[1] < 0 && p.damaged() >= 0) info[1] = d.bands() + p.damaged();
    d.down(rp, partials); d.down(rs, sum); d.down(rst, state); d.down(rp2, partials2); d.down(rs2, sums2); d.down(rst2, st2);
    p.down(pst, host_state);
    return 0;
}

// mir_lsq_unpack_grad_*: ONE jtj_unpack (k_unpack_grad on n + 1 workgroups of 128 threads) on a packed buffer and a state image
template <typename T>
int unpack_grad_entry(size_t n_, const T* packed, void* state, T* JJ, T* Jy, int info[2])
{
    if (!packed || !state || !JJ || !Jy || !info || n_ == 0 || n_ > 4096) return -1;
    if (!device_available()) return -2;
    const int n = (int)n_;
    Banded d;
    const size_t rp = d.take(n_ * (n_ + 1) / 2 + n_, sizeof(T)), rJJ = d.take(n_ * n_, sizeof(T)), rJy = d.take(n_, sizeof(T)),
                 rst = d.take(1, sizeof(LmState<T>));
    if (!d.alloc() || !d.up(rp, packed) || !d.up(rst, state)) return -3;
    if (jtj_unpack<T>((const T*)d.at(rp), n, (T*)d.at(rJJ), (T*)d.at(rJy), (LmState<T>*)d.at(rst), nullptr) != hipSuccess) {
        (void)hipDeviceSynchronize();
        return -4;
    }
    if (!launches_done() || !d.fetch()) return -5;
    info[0] = d.damaged(); info[1] = d.bands();
    d.down(rJJ, JJ); d.down(rJy, Jy); d.down(rst, state);
    return 0;
}

// The body of mir_lsq_jtj_* / mir_lsq_fd_jtj_d / mir_lsq_fd_diff_jtj_d: ONE jtj_run of `op` on the caller's operands in `a` (the call
// adds the slabs and, for the rewrite, ||dx||^2) and jtj_unpack; kernel_ms brackets jtj_run alone.
template <typename T>
int jtj_entry(JtjOp op, JtjArgs<T> a, T* JJ, T* Jy, void* stream_, float* kernel_ms)
{
    if (!device_available()) return -1;
    if (a.n == 0 || a.m == 0) return -2;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const JtjPlan plan = jtj_plan<T>(a.m, a.n, query_num_cu());
    if (plan.of(op).kernel == JtjKernel::none) return -6;   // shape not covered by a fused kernel
    const size_t n = (size_t)a.n, packed_len = n * (n + 1) / 2 + n + 8;
    T* packed = nullptr;
    LmState<T>* st = nullptr;
    if (hipMalloc((void**)&a.slabs, sizeof(T) * jtj_slab_elems(plan)) != hipSuccess) return -3;
    if (hipMalloc((void**)&packed, sizeof(T) * packed_len) != hipSuccess) { (void)hipFree(a.slabs); return -3; }
    if (hipMalloc((void**)&st, sizeof(LmState<T>) + sizeof(T) * 8) != hipSuccess) { (void)hipFree(a.slabs); (void)hipFree(packed); return -3; }
    int rc = 0;
    if (op == JtjOp::rewrite) {
        // ||dx||^2 on the device (n-vector, one block)
        T* dxdot = reinterpret_cast<T*>(st + 1);
        hipLaunchKernelGGL(k_sumsq_partial<T>, dim3(1), dim3(256), 0, stream, a.dx, n, packed);
        hipLaunchKernelGGL(k_sumsq_final<T>, dim3(1), dim3(256), 0, stream, packed, 1, dxdot);
        a.dx_dot = dxdot;
    }
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, stream);
    if (jtj_run<T>(plan, op, a, packed, stream) != hipSuccess) rc = -4;
    (void)hipEventRecord(e1, stream);
    (void)jtj_unpack<T>(packed, (int)n, JJ, Jy, st, stream);
    if (hipStreamSynchronize(stream) != hipSuccess) rc = -5;
    if (kernel_ms) { float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1); *kernel_ms = ms; }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(a.slabs); (void)hipFree(packed); (void)hipFree(st);
    return rc;
}
template <typename T>
int plain_jtj_entry(size_t m, size_t n, T* J, const T* y, const T* y_old, const T* dx, int broyden, T* JJ, T* Jy, void* stream, float* kernel_ms)
{
    JtjArgs<T> a{};
    a.J = J; a.Jout = J; a.y = y; a.y_old = y_old; a.dx = dx; a.m = m; a.n = (int)n;
    return jtj_entry<T>(broyden ? JtjOp::rewrite : JtjOp::plain, a, JJ, Jy, stream, kernel_ms);
}
// op: fd (Yrm the pair panel), fd_diff (the difference panel) or, J == NULL, fd_diff_keep
int fd_jtj_entry(JtjOp op, size_t m, size_t n, const double* Yrm, const double* twh, const double* y, double* J, double* JJ, double* Jy,
                 void* stream, float* kernel_ms)
{
    JtjArgs<double> a{};
    a.J = Yrm; a.Jout = J; a.y = y; a.y_old = y; a.m = m; a.n = (int)n; a.twh = twh;
    return jtj_entry<double>(op, a, JJ, Jy, stream, kernel_ms);
}
}  // namespace

extern "C" {

int mir_solve_box_qp_gpu_d(const mir_box_qp_settings_d* settings, size_t n, const double* P, const double* q,
                           const double* l, const double* u, double* x, int unconstrainedSolution, int* iterations)
{
    return box_qp_entry<double>(settings, n, P, q, l, u, x, unconstrainedSolution, iterations);
}
int mir_solve_box_qp_gpu_s(const mir_box_qp_settings_s* settings, size_t n, const float* P, const float* q,
                           const float* l, const float* u, float* x, int unconstrainedSolution, int* iterations)
{
    return box_qp_entry<float>(settings, n, P, q, l, u, x, unconstrainedSolution, iterations);
}

int mir_lsq_jtj_d(size_t m, size_t n, double* J, const double* y, const double* y_old, const double* dx, int broyden,
                  double* JJ, double* Jy, void* stream, float* kernel_ms)
{
    return plain_jtj_entry<double>(m, n, J, y, y_old, dx, broyden, JJ, Jy, stream, kernel_ms);
}
int mir_lsq_fd_jtj_d(size_t m, size_t n, const double* Yrm, const double* twh, const double* y, double* J,
                     double* JJ, double* Jy, void* stream_, float* kernel_ms)
{
    return fd_jtj_entry(JtjOp::fd, m, n, Yrm, twh, y, J, JJ, Jy, stream_, kernel_ms);
}
int mir_lsq_fd_diff_jtj_d(size_t m, size_t n, const double* Drm, const double* twh, const double* y, double* J,
                          double* JJ, double* Jy, void* stream_, float* kernel_ms)
{
    return fd_jtj_entry(J ? JtjOp::fd_diff : JtjOp::fd_diff_keep, m, n, Drm, twh, y, J, JJ, Jy, stream_, kernel_ms);
}
int mir_lsq_jtj_plan(size_t elem_size, size_t m, size_t n, int num_cu, int op, int aligned16, size_t out[10])
{
    if ((elem_size != 4 && elem_size != 8) || m == 0 || n == 0 || n > (size_t)1 << 20 || num_cu < 1 || op < 0 || op > 4 || !out) return -1;
    const JtjPlan p = elem_size == 8 ? jtj_plan<double>(m, (int)n, num_cu) : jtj_plan<float>(m, (int)n, num_cu);
    const JtjLaunch l = jtj_resolve(p, (JtjOp)op, aligned16 != 0);
    const bool wide = l.kernel == JtjKernel::wide;
    const size_t v[10] = {(size_t)l.kernel, (size_t)l.ncb, (size_t)l.flat, (size_t)l.nblk, (size_t)l.njobs, l.lds,
                          (size_t)l.nblk * l.njobs, (size_t)l.slab_len, wide ? 0 : (size_t)l.ncb, jtj_slab_elems(p)};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return 0;
}
int mir_lsq_lm_solve_d(const mir_least_squares_settings_d* settings, size_t n, double* JJ, double* Jy, double* x, double* lower,
                       double* upper, int ks, const double* lam, double state_lambda, unsigned mode, mir_lsq_lm_solve_record_d* rec,
                       double* dx, double* trial, double* jy_inf, int info[6])
{
    return lm_solve_entry<double>(settings, n, JJ, Jy, x, lower, upper, ks, lam, state_lambda, mode, rec, dx, trial, jy_inf, info);
}
int mir_lsq_lm_solve_s(const mir_least_squares_settings_s* settings, size_t n, float* JJ, float* Jy, float* x, float* lower,
                       float* upper, int ks, const float* lam, float state_lambda, unsigned mode, mir_lsq_lm_solve_record_s* rec,
                       float* dx, float* trial, float* jy_inf, int info[6])
{
    return lm_solve_entry<float>(settings, n, JJ, Jy, x, lower, upper, ks, lam, state_lambda, mode, rec, dx, trial, jy_inf, info);
}
int mir_lsq_lm_solve_class(size_t elem_size, size_t n, int bounded, int generic, int diagnostic, int out[3])
{
    if ((elem_size != 4 && elem_size != 8) || n == 0 || n > (size_t)1 << 20 || !out) return -1;
    const LmSolveClass c = lm_solve_class((int)elem_size, (int)n, bounded != 0, generic != 0, diagnostic != 0);
    out[0] = c.kind; out[1] = c.nb; out[2] = c.bounded;
    return 0;
}
int mir_lsq_lr_pass_d(size_t m, size_t n, int k, const double* J, double* U, double* D, const double* dx, const double* dx_dot,
                      const double* y, int count, const double* y_old, double* JJ, double* Jy, const mir_lsq_lm_solve_record_d* spec,
                      double absTolerance, double relTolerance, double* partials, double* reduced, double* sums, double* jy_inf,
                      int info[6])
{
    return lr_pass_entry<double>(m, n, k, J, nullptr, U, D, dx, dx_dot, y, count, y_old, JJ, Jy, spec, absTolerance, relTolerance, partials,
                                 reduced, sums, jy_inf, info);
}
int mir_lsq_lr_pass_s(size_t m, size_t n, int k, const float* J, float* U, float* D, const float* dx, const float* dx_dot,
                      const float* y, int count, const float* y_old, float* JJ, float* Jy, const mir_lsq_lm_solve_record_s* spec,
                      float absTolerance, float relTolerance, float* partials, float* reduced, float* sums, float* jy_inf,
                      int info[6])
{
    return lr_pass_entry<float>(m, n, k, J, nullptr, U, D, dx, dx_dot, y, count, y_old, JJ, Jy, spec, absTolerance, relTolerance, partials,
                                reduced, sums, jy_inf, info);
}
int mir_lsq_lr_pass_scaled_d(size_t m, size_t n, int k, const double* P, const double* twh, double* U, double* D, const double* dx,
                             const double* dx_dot, const double* y, int count, const double* y_old, double* JJ, double* Jy,
                             const mir_lsq_lm_solve_record_d* spec, double absTolerance, double relTolerance, double* partials,
                             double* reduced, double* sums, double* jy_inf, int info[6])
{
    if (!twh || n > (size_t)kLrScaledMaxN) return -1;
    return lr_pass_entry<double>(m, n, k, P, twh, U, D, dx, dx_dot, y, count, y_old, JJ, Jy, spec, absTolerance, relTolerance, partials,
                                 reduced, sums, jy_inf, info);
}
int mir_lsq_lr_flush_scaled_d(size_t m, size_t n, int k, double* J, const double* P, const double* twh, const double* U, const double* D,
                              int info[2])
{
    if (!J || !P || !twh || !U || !D || !info || m == 0 || n == 0 || n > (size_t)kLrScaledMaxN || k < 1 || k > kLrMax) return -1;
    if (!device_available()) return -2;
    const LrClass cls = lr_class((int)n, reinterpret_cast<uintptr_t>(J) % 16 == 0 && reinterpret_cast<uintptr_t>(P) % 16 == 0);
    info[0] = cls.ncp; info[1] = cls.vec;
    if (lr_flush_scaled(J, P, twh, U, D, k, m, (int)n, query_num_cu(), nullptr) != hipSuccess) { (void)hipDeviceSynchronize(); return -4; }
    return hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess ? 0 : -5;
}
int mir_lsq_lr_flush_d(size_t m, size_t n, int k, double* J, const double* U, const double* D, int info[2])
{
    return lr_flush_entry<double>(m, n, k, J, U, D, info);
}
int mir_lsq_lr_flush_s(size_t m, size_t n, int k, float* J, const float* U, const float* D, int info[2])
{
    return lr_flush_entry<float>(m, n, k, J, U, D, info);
}
int mir_lsq_lr_class(size_t elem_size, size_t n, int aligned, int out[2])
{
    if ((elem_size != 4 && elem_size != 8) || n == 0 || n > (size_t)kLrMaxN || !out) return -1;
    const LrClass c = lr_class((int)n, aligned != 0);
    out[0] = c.ncp; out[1] = c.vec;
    return 0;
}
int mir_lsq_lr_blocks(size_t m, int num_cu)
{
    if (m == 0) return -1;
    if (num_cu <= 0) {
        if (!device_available()) return -2;
        num_cu = query_num_cu();
    }
    return lr_blocks(m, num_cu);
}
int mir_lsq_decide_d(const mir_least_squares_settings_d* settings, size_t n, int ks, unsigned mode, uint32_t maxIterations, uint32_t seq,
                     mir_lsq_lm_state_d* state, mir_lsq_lm_solve_record_d* rec, double* sums, double* x, double* trial, double* dx_chain,
                     double* dx_acc, double* partials, int nparts, int pstride, mir_lsq_lm_state_d* host_state, double* host_x, int info[2])
{
    return decide_entry<double>(settings, n, ks, mode, maxIterations, seq, state, rec, sums, x, trial, dx_chain, dx_acc, partials, nparts,
                                pstride, host_state, host_x, info);
}
int mir_lsq_decide_s(const mir_least_squares_settings_s* settings, size_t n, int ks, unsigned mode, uint32_t maxIterations, uint32_t seq,
                     mir_lsq_lm_state_s* state, mir_lsq_lm_solve_record_s* rec, float* sums, float* x, float* trial, float* dx_chain,
                     float* dx_acc, float* partials, int nparts, int pstride, mir_lsq_lm_state_s* host_state, float* host_x, int info[2])
{
    return decide_entry<float>(settings, n, ks, mode, maxIterations, seq, state, rec, sums, x, trial, dx_chain, dx_acc, partials, nparts,
                               pstride, host_state, host_x, info);
}
int mir_lsq_fd_points_d(size_t n, const double* x, const double* lower, const double* upper, double eps, int with_base, double* X,
                        double* twh, double* twh_host, int info[2])
{
    return fd_points_entry<double>(n, x, lower, upper, eps, with_base, X, twh, twh_host, info);
}
int mir_lsq_fd_points_s(size_t n, const float* x, const float* lower, const float* upper, float eps, int with_base, float* X,
                        float* twh, float* twh_host, int info[2])
{
    return fd_points_entry<float>(n, x, lower, upper, eps, with_base, X, twh, twh_host, info);
}
int mir_lsq_fd_fill_d(size_t m, size_t n, size_t ldy, int j0, int pc, const double* Y, const double* twh, double* J, int col, int info[2])
{
    return fd_fill_entry<double>(m, n, ldy, j0, pc, Y, twh, J, col, info);
}
int mir_lsq_fd_fill_s(size_t m, size_t n, size_t ldy, int j0, int pc, const float* Y, const float* twh, float* J, int col, int info[2])
{
    return fd_fill_entry<float>(m, n, ldy, j0, pc, Y, twh, J, col, info);
}
int mir_lsq_entry_state_d(size_t m, const double* v, uint32_t seq, double* partials, double* sum, mir_lsq_lm_state_d* state,
                          mir_lsq_lm_state_d* host_state, double* partials2, double* sums2, mir_lsq_lm_state_d* st2, int info[3])
{
    return entry_state_entry<double>(m, v, seq, partials, sum, state, host_state, partials2, sums2, st2, info);
}
int mir_lsq_entry_state_s(size_t m, const float* v, uint32_t seq, float* partials, float* sum, mir_lsq_lm_state_s* state,
                          mir_lsq_lm_state_s* host_state, float* partials2, float* sums2, mir_lsq_lm_state_s* st2, int info[3])
{
    return entry_state_entry<float>(m, v, seq, partials, sum, state, host_state, partials2, sums2, st2, info);
}
int mir_lsq_sumsq_blocks(size_t m) { return m ? sumsq_blocks(m) : -1; }
int mir_lsq_unpack_grad_d(size_t n, const double* packed, mir_lsq_lm_state_d* state, double* JJ, double* Jy, int info[2])
{
    return unpack_grad_entry<double>(n, packed, state, JJ, Jy, info);
}
int mir_lsq_unpack_grad_s(size_t n, const float* packed, mir_lsq_lm_state_s* state, float* JJ, float* Jy, int info[2])
{
    return unpack_grad_entry<float>(n, packed, state, JJ, Jy, info);
}
int mir_lsq_jtj_s(size_t m, size_t n, float* J, const float* y, const float* y_old, const float* dx, int broyden,
                  float* JJ, float* Jy, void* stream, float* kernel_ms)
{
    return plain_jtj_entry<float>(m, n, J, y, y_old, dx, broyden, JJ, Jy, stream, kernel_ms);
}
int mir_lsq_selftest_reductions(int rounds, int mismatches[4])
{
    if (!mismatches || rounds <= 0) return -1;
    if (!device_available()) return -2;
    int* d = nullptr;
    if (hipMalloc((void**)&d, 4 * sizeof(int)) != hipSuccess) return -3;
    bool ok = hipMemset(d, 0, 4 * sizeof(int)) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_selftest_reductions, dim3(2048), dim3(256), 0, nullptr, rounds, 12345u, d);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess
          && hipMemcpy(mismatches, d, 4 * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d);
    return ok ? 0 : -4;
}

// the callbacks of mir_fit_spline_gpu_* one call at a time, their host twins and the knots' factor (fit_spline_gpu.hip)
int mir_fit_spline_gpu_eval_d(size_t npoints, const double* points, size_t nx, const double* x, double lambda, size_t p,
                              const double* X, int mode, double* out)
{
    return spline_gpu::callback_eval<double>(npoints, points, nx, x, lambda, p, X, mode, out);
}
int mir_fit_spline_gpu_eval_s(size_t npoints, const float* points, size_t nx, const float* x, float lambda, size_t p,
                              const float* X, int mode, float* out)
{
    return spline_gpu::callback_eval<float>(npoints, points, nx, x, lambda, p, X, mode, out);
}
int mir_fit_spline_eval_host_d(size_t npoints, const double* points, size_t nx, const double* x, double lambda, size_t p,
                               const double* X, int mode, double* out)
{
    return spline_gpu::host_eval<double>(npoints, points, nx, x, lambda, p, X, mode, out);
}
int mir_fit_spline_eval_host_s(size_t npoints, const float* points, size_t nx, const float* x, float lambda, size_t p,
                               const float* X, int mode, float* out)
{
    return spline_gpu::host_eval<float>(npoints, points, nx, x, lambda, p, X, mode, out);
}
int mir_fit_spline_factor_d(size_t nx, const double* x, double* F) { return spline_gpu::factor<double>(nx, x, F); }
int mir_fit_spline_factor_s(size_t nx, const float* x, float* F) { return spline_gpu::factor<float>(nx, x, F); }

}  // extern "C"
