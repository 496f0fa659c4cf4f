// workloads_gemm.hip -- the batched tanh-linear residual of the synthetic workloads as a tall GEMM on the f64 matrix cores
// (caller side of the boundary, like workloads.hip: the role of the user's batched f, mir_lsq_batched_function_d).
#include "workloads_gemm.h"
#include "workloads_device.h"

namespace {

// ---- batched tanh-linear residuals: Y[p][i] = tanh(a_i . X[p]) - b_i for p < P points in ONE
//      sweep over A (the finite-difference Jacobian evaluates its 2n perturbed points together).
//      It is a tall GEMM A[m x n] X^T[n x P] on v_mfma_f64_16x16x4_f64:
//        * workgroup = 16 waves; wave w owns points [16 w, 16 w + 16) of a 256-point chunk and keeps
//          their X fragments (B operand, NK k-steps) in registers for the whole sweep;
//        * the workgroup streams 16-row tiles of A through a double-buffered, padded LDS image
//          (row pitch n + 2 doubles -> the 16-row x 4-column A-operand read is bank-conflict free);
//          every byte of A is read from HBM once per 256 points;
//        * epilogue: tanh - b on the accumulator, stored along the row index (4 x 32-byte runs per
//          point and tile, merged into full lines in L2).
template <int NK>
__global__ __launch_bounds__(1024) void k_tanh_linear_batched(const double* __restrict__ A, const double* __restrict__ b,
                                                               const double* __restrict__ X, double* __restrict__ Y,
                                                               size_t m, int n, int P)
{
    using Acc = __attribute__((ext_vector_type(4))) double;
    constexpr int NPAD = 4 * NK;            // padded column count
    constexpr int PITCH = NPAD + 2;         // doubles
    __shared__ __attribute__((aligned(16))) double tile[2][16 * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;

    // zero the padding columns once (never overwritten afterwards)
    for (int idx = tid; idx < 2 * 16 * PITCH; idx += 1024) (&tile[0][0])[idx] = 0.0;
    __syncthreads();

    // piece -> (row, 16-byte column pair) of a 16-row tile; tile rows are contiguous in memory
    const int ppr = n / 2;                  // 16-byte pieces per row (n even)
    const bool has_piece = tid < 16 * ppr;
    const int prow = has_piece ? tid / ppr : 0, pcol = has_piece ? tid % ppr : 0;
    const size_t ntiles = (m + 15) / 16;

    for (int pbase = 0; pbase < P; pbase += 256) {
        const int pl = pbase + wave * 16 + fr;                  // this lane's point
        const bool pok = pl < P;
        const bool wave_active = pbase + wave * 16 < P;         // wave-uniform
        double xf[NK];
#pragma unroll
        for (int s = 0; s < NK; ++s) {
            const int col = 4 * s + fq;
            xf[s] = (pok && col < n) ? X[(size_t)pl * n + col] : 0.0;
        }
        double2 stage = make_double2(0.0, 0.0);
        auto gload = [&](size_t t) {
            const size_t row = t * 16 + prow;
            if (has_piece && row < m) stage = *reinterpret_cast<const double2*>(A + row * (size_t)n + 2 * pcol);
            else stage = make_double2(0.0, 0.0);
        };
        auto lstore = [&](int buf) {
            if (has_piece) *reinterpret_cast<double2*>(&tile[buf][prow * PITCH + 2 * pcol]) = stage;
        };
        size_t t = blockIdx.x;
        if (t < ntiles) { gload(t); lstore(0); }
        if (t + gridDim.x < ntiles) gload(t + gridDim.x);
        __syncthreads();
        int buf = 0;
        // software pipeline over tiles: the tanh / store epilogue of tile t - 1 is independent VALU work placed in
        // the same basic block as the (dependent, latency-bound) MFMA chain of tile t, so the scheduler overlaps them
        Acc prev = {0.0, 0.0, 0.0, 0.0};
        size_t tprev = ntiles;                                  // "no previous tile"
        auto epilogue = [&](const Acc& acc, size_t tt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t row = tt * 16 + fq + 4 * r;
                if (pok && tt < ntiles && row < m) Y[(size_t)pl * m + row] = dtanh(acc[r]) - b[row];
            }
        };
        for (; t < ntiles; t += gridDim.x) {
            if (wave_active) {                                  // waves whose 16 points are all >= P only help staging
                Acc acc = {0.0, 0.0, 0.0, 0.0};
                const double* tp = &tile[buf][fr * PITCH + fq];
#pragma unroll
                for (int s = 0; s < NK; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(tp[4 * s], xf[s], acc, 0, 0, 0);
                epilogue(prev, tprev);                          // D: col = lane & 15 = point, row = (lane >> 4) + 4 r
                prev = acc;
                tprev = t;
            }
            // stage tile t + grid into the other buffer (its last readers passed the previous barrier)
            if (t + gridDim.x < ntiles) lstore(buf ^ 1);
            if (t + 2 * (size_t)gridDim.x < ntiles) gload(t + 2 * (size_t)gridDim.x);
            __syncthreads();
            buf ^= 1;
        }
        if (wave_active) epilogue(prev, tprev);
        __syncthreads();
    }
}


// ---- batched residuals, LDS-DMA version (n = 32, 64, 128): same GEMM, restructured like the solver's J^T J kernel.
//      The first version above stages A through VGPRs and its waves wait, every 16-row tile, on a vmcnt that also
//      covers their own scattered Y stores (measured 2.1 ms for m = 1e6, n = p = 128: 15 TFLOP/s). Here
//        * waves 0..7 compute (wave w owns points [16 w, 16 w + 16) of a 128-point chunk) and issue NO loads in the
//          sweep: their Y stores are fire-and-forget;
//        * waves 8, 9 only issue `global_load_lds_dwordx4` DMA into a ring of NS stages of 32 rows (D stages in flight,
//          counted vmcnt over DMA only, one raw s_barrier per stage); b rides in a small ring of its own;
//        * LDS layout: row-major without padding, 16-byte pieces XOR-swizzled with the row (the DMA picks the SOURCE
//          row and piece per lane, the LDS side of a DMA is always lane x 16 B). The K index of the MFMA chain is
//          permuted so that one ds_read_b128 (4 LDS cycles, conflict-free with this swizzle) is the A operand of two
//          k-steps; ds_read2_b64, which the compiler forms from paired 8-byte reads, costs 8 cycles and 2-way conflicts;
//        * LDS row i of a tile holds memory row rho(i), so that a lane's four accumulator rows are two adjacent row
//          pairs: the epilogue stores 16-byte pairs, 64 contiguous bytes per point and instruction;
//        * two independent accumulator chains (two 16-row tiles of the stage) per wave keep the MFMA pipe full; the two
//          compute waves of a SIMD run out of phase (MFMA-then-epilogue vs epilogue-then-MFMA).
typedef __attribute__((address_space(3))) void* wl_lds_ptr;
typedef const __attribute__((address_space(1))) void* wl_gbl_ptr;

// MFMA row i of a 16-row tile holds memory row rho(i): D row fq + 4 r  <->  memory row (r >> 1) * 8 + 2 fq + (r & 1)
__device__ __forceinline__ constexpr int tlb_rho(int i) { return ((i >> 2) >> 1) * 8 + 2 * (i & 3) + ((i >> 2) & 1); }
// 16-byte piece p of LDS row i is stored at piece position p ^ sigma(i): with it the 4 x 16-lane groups of a
// ds_read_b128 A-operand fetch ({0-3, 12-15, 20-27}, ...) each touch 16 distinct 16-byte bank slots
__device__ __forceinline__ constexpr int tlb_sigma(int i) { return (i + 12) & 15; }

template <int NK> struct TlbCfg {
    static constexpr int N = 4 * NK;
    static constexpr int PPR = N / 2;                       // 16-byte pieces per row
    // n <= 128: 8 compute waves x 16 points, two 16-row tiles per stage (two MFMA chains per wave), 168 VGPRs;
    // n = 256: the X fragments alone are 128 VGPRs -> 8 waves per workgroup (256 VGPRs each), one tile per stage with the
    // K range split over two accumulator chains
    static constexpr int TILES = NK <= 32 ? 2 : 1;
    // SELF (n = 256): no loader waves -- eight compute waves (two per SIMD, as at n <= 128) each issue an eighth of a stage's DMA
    // and wait for it with a count over the YOUNGER DMA only (see tlb_compute); with two loader waves among eight, two SIMDs
    // carried one compute wave and the MFMA pipe could not pass 0.75 (measured 0.59, A swept six times for 512 points)
    static constexpr bool SELF = NK > 32;
    static constexpr int COMPUTE_WAVES = 8, LOADER_WAVES = SELF ? 0 : 2;
    static constexpr int CHUNK = 16 * COMPUTE_WAVES;        // points per sweep over A
    static constexpr int ROWS = 16 * TILES;                 // rows per stage
    static constexpr int STAGE_BYTES = ROWS * N * 8;
    static constexpr int IPS = STAGE_BYTES / 1024;          // 1 KB DMA instructions per stage
    static constexpr int NS = 4, D = 2, NSB = 8;
    static constexpr int B_OFF = NS * STAGE_BYTES;
    static constexpr int LDS_BYTES = B_OFF + NSB * 256;
    static constexpr int THREADS = 64 * (COMPUTE_WAVES + LOADER_WAVES);
    // prefix-forking difference panel (n = 128, tlb_fork_*): the base chain's accumulators P_2, P_4, ..., P_{NK-2} of both
    // tiles of a stage, 16 doubles each in the D layout [fq][r], in a two-stage ring behind the b ring; then the vote word
    static constexpr bool FORK = NK == 32;
    static constexpr int NPRE = NK / 2 - 1;
    static constexpr int PRE_STAGE = TILES * NPRE * 16 * 8;
    static constexpr int PRE_OFF = LDS_BYTES;
    static constexpr int VOTE_OFF = PRE_OFF + 2 * PRE_STAGE;
    static constexpr int FORK_LDS_BYTES = VOTE_OFF + 16;
    // the extra point of fbRowMajorDiff with p = 2n + 1 (BASE instances, n = 128): its n coordinates behind the vote word
    static constexpr int BASE_OFF = FORK_LDS_BYTES;
    static constexpr int BASE_LDS_BYTES = BASE_OFF + N * 8;
};

// ---- the extra point of a p = 2n + 1 call (n = 128): its residual for the 32 rows of the stage in `slot`, in eight shares of
//      four LDS rows (`wave` names the share; tlb_fork_compute says which wave takes which), each one wave's work,
//      with the arithmetic of the one-point sweep k_tanh_linear<double, 4, 0, true> -- 16 lanes per row,
//      lane p the column pairs 32 c + 2 p, + 1 (piece 16 c + p of the row, at position 16 c + (p ^ sigma) of its LDS image),
//      tanh_linear_row_sum, sum16, dtanh, - b: bit for bit what that kernel writes. (The base chain of the loader waves sums the
//      same products in the MFMA's order; it cannot serve.) LDS row R holds memory row (R & 16) + rho(R & 15) of the stage.
// the lane number, formed where it is asked for (volatile: not hoisted, not merged with the kernel's own copy)
__device__ __forceinline__ int tlb_lane_now()
{
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
template <int NK>
__device__ __forceinline__ void tlb_base_rows(const unsigned char* slot, const unsigned char* bslot, const unsigned char* smem,
                                              double* __restrict__ ybase, size_t row0, size_t m, int wave)
{
    using C = TlbCfg<NK>;
    static_assert(C::N == 128 && C::ROWS == 32 && C::COMPUTE_WAVES == 8, "four rows a wave, four column pairs a lane");
    // The forked kernel runs at its register limit (168): everything here that depends on the lane is formed again per stage from
    // a lane number the optimiser cannot see through -- a dozen integer operations -- instead of living in registers across the
    // MFMA chains and the epilogues (hoisted, the addresses below and three of dtanh's constants went to scratch memory, whose
    // reloads wait behind the epilogue's stores); the row bound and the store's base are wave-uniform.
    const int lane = tlb_lane_now();
    const int q = lane >> 4, p = lane & 15;
    const int R = 4 * wave + q;
    const unsigned char* rp = slot + R * C::N * 8 + (p ^ tlb_sigma(R & 15)) * 16;
    const unsigned char* xp = smem + C::BASE_OFF + p * 16;
    // two column pairs at a time (the same sum, c ascending): 16 registers of operands in flight instead of 32
    double s = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        double v0[2], v1[2], x0[2], x1[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const double2 a = *reinterpret_cast<const double2*>(rp + (2 * h + c) * 256);
            const double2 x = *reinterpret_cast<const double2*>(xp + (2 * h + c) * 256);
            v0[c] = a.x; v1[c] = a.y;
            x0[c] = x.x; x1[c] = x.y;
        }
        s = tanh_linear_row_sum<double, 2>(v0, v1, x0, x1, s);
        __builtin_amdgcn_sched_barrier(0);
    }
    s = sum16(s);
    const double t = dtanh(s);
    const int lr = (R & 16) + tlb_rho(R & 15);
    const double bv = *reinterpret_cast<const double*>(bslot + lr * 8);
    const int rows = m - row0 < (size_t)C::ROWS ? (int)(m - row0) : C::ROWS;      // rows of the stage that exist (row0 < m)
    if (p == 0 && lr < rows) (ybase + row0)[lr] = t - bv;
}

// The two 16-point groups of compute wave w in the forked kernel (which = 0: the one that forks first). Group g costs
// 32 - 2 g k-steps per tile, and the waves w, w + 4 share SIMD w % 4; the loader waves 8, 9 sit on SIMDs 0 and 1. The table
// is chosen by measurement: the SIMDs that also carry a loader get 60 k-steps per tile (30 per wave), the other two 76
// (38 per wave). Tables with 56, 58, 62 and 64 on the loader SIMDs were each 1 to 3 % slower (DESIGN section 3,
// profiles/r16): a loader's DMA issue and waits cost its SIMD more than its instruction count says.
// tlb_fork_vote and tlb_fork_compute both read the table.
__host__ __device__ constexpr int tlb_fork_group(int w, int which)
{
    constexpr int T[8][2] = {{2, 15}, {3, 14}, {0, 13}, {1, 12}, {6, 11}, {7, 10}, {4, 9}, {5, 8}};
    return T[w][which];
}
constexpr bool tlb_fork_groups_ok()
{
    int owners[16] = {};
    for (int w = 0; w < 8; ++w) {
        if (tlb_fork_group(w, 0) >= tlb_fork_group(w, 1)) return false;        // tlb_fork_compute starts the second group inside the first's loop
        for (int which = 0; which < 2; ++which) {
            const int g = tlb_fork_group(w, which);
            if (g < 0 || g > 15) return false;
            ++owners[g];
        }
    }
    for (int g = 0; g < 16; ++g)
        if (owners[g] != 1) return false;
    return true;
}
static_assert(tlb_fork_groups_ok(), "every 16-point group 0..15 belongs to exactly one compute wave");

// loader LOADER's share of the DMA of flat stage f (f % S of this workgroup's stages) into ring slot f % NS; loader 1 also b
template <int NK, int LOADER>
__device__ __forceinline__ void tlb_issue(const double* __restrict__ A, const double* __restrict__ b, size_t m,
                                          unsigned char* smem, int lane, size_t S, size_t f)
{
    using C = TlbCfg<NK>;
    constexpr int MYI = C::IPS / 2;
    const unsigned char* Ab = reinterpret_cast<const unsigned char*>(A);
    const unsigned char* bb = reinterpret_cast<const unsigned char*>(b);
    const size_t stage = blockIdx.x + (f % S) * (size_t)gridDim.x;
    const size_t row0 = stage * C::ROWS;
    unsigned char* slot = smem + (f % C::NS) * C::STAGE_BYTES;
#pragma unroll
    for (int k = 0; k < MYI; ++k) {
        const int ins = LOADER + 2 * k;
        const int g = ins * 64 + lane;                          // 16-byte piece of the stage image this lane fills
        const int R = g / C::PPR, sp = g % C::PPR;              // LDS row within the stage = 16 tile + MFMA row
        size_t row = row0 + (R & 16) + tlb_rho(R & 15);         // the memory row that feeds it
        row = row < m ? row : m - 1;                            // rows past m: valid bytes, never stored
        const int piece = sp ^ tlb_sigma(R & 15);
        __builtin_amdgcn_global_load_lds((wl_gbl_ptr)(Ab + (row * C::N + 2 * piece) * 8),
                                         (wl_lds_ptr)(slot + ins * 1024), 16, 0, 2 /* nt */);
    }
    if constexpr (LOADER == 1) {
        size_t row = row0 + (lane >> 1);
        row = row < m ? row : m - 1;
        __builtin_amdgcn_global_load_lds((wl_gbl_ptr)(bb + row * 8 + (lane & 1) * 4),
                                         (wl_lds_ptr)(smem + C::B_OFF + (f % C::NSB) * 256), 4, 0, 0);
    }
}

template <int NK, int LOADER>
__device__ __forceinline__ void tlb_loader(const double* __restrict__ A, const double* __restrict__ b, size_t m,
                                           unsigned char* smem, int lane, size_t S, size_t F)
{
    using C = TlbCfg<NK>;
    constexpr int OPS = C::IPS / 2 + (LOADER == 1 ? 1 : 0);
    auto issue = [&](size_t f) { tlb_issue<NK, LOADER>(A, b, m, smem, lane, S, f); };
    const size_t pre = F < (size_t)C::D ? F : (size_t)C::D;
    for (size_t f = 0; f < pre; ++f) issue(f);
    for (size_t f = 0; f < F; ++f) {
        if (f + C::D < F) {
            issue(f + C::D);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::D * OPS) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
    }
}

// RM: Y is m x P row-major (point k's residual of row i at Y[i P + k]; 16 lanes of a row = 128 contiguous bytes) --
// the layout the solver's fused finite-difference J^T J kernel consumes (mir_lsq_gpu_options.fbRowMajor)
// DIFF (with RM): points come in (+h, -h) pairs (2 j, 2 j + 1) -- adjacent lanes -- and Y is the m x P/2 row-major DIFFERENCE
// panel D[i][j] = y_{2j}[i] - y_{2j+1}[i] (mir_lsq_gpu_options.fbRowMajorDiff): the even lane of a pair subtracts its
// neighbour's residual (a DPP move) and stores; half the panel bytes of RM
template <int NK, bool ALIGNED, int GROUP, bool RM = false, bool DIFF = false>
__device__ __forceinline__ void tlb_compute(const double* __restrict__ A, const double* __restrict__ b,
                                            const double* __restrict__ X, double* __restrict__ Y, size_t m, int P,
                                            unsigned char* smem, int lane, int wave, size_t S, int nchunks)
{
    using C = TlbCfg<NK>;
    using Acc = __attribute__((ext_vector_type(4))) double;
    const int fr = lane & 15, fq = lane >> 4;
    // k-step s = 2 j + e of the MFMA chain multiplies column 8 j + 2 fq + e: one ds_read_b128 (piece 4 j + fq of LDS
    // row fr) feeds two k-steps, and X is read as the matching column pairs
    const int v = fq ^ tlb_sigma(fr);
    int laddr[4];                                               // byte offsets of j = 0..3 (mod 4) in a stage
#pragma unroll
    for (int k = 0; k < 4; ++k) laddr[k] = fr * C::N * 8 + ((4 * k) ^ v) * 16;

    // SELF: this wave's share of the DMA (instructions wave, wave + 8, ... of a stage; wave 0 also b). Loads return in issue
    // order among themselves, stores do not keep order with loads: a count of the YOUNGER LOADS ONLY is a safe wait for a
    // stage (if one of its loads were pending, so would be every younger one: more than the count) -- pending stores can only
    // make it wait longer, and the wait sits before the epilogue's stores, behind a stage's worth of matrix-core work.
    constexpr int MYI = C::SELF ? C::IPS / C::COMPUTE_WAVES : 1;
    [[maybe_unused]] int roff[MYI], soff[MYI];
    [[maybe_unused]] unsigned is_next = 0, slot_next = 0, bslot_next = 0;          // stage (of S), ring slot, b slot of the next issue
    [[maybe_unused]] const size_t Ftot = S * (size_t)nchunks;
    [[maybe_unused]] size_t fissued = 0;
    const unsigned char* Ab = reinterpret_cast<const unsigned char*>(A);
    const unsigned char* bb = reinterpret_cast<const unsigned char*>(b);
    if constexpr (C::SELF) {
#pragma unroll
        for (int k = 0; k < MYI; ++k) {
            const int g = (wave + C::COMPUTE_WAVES * k) * 64 + lane;
            const int R = g / C::PPR, sp = g % C::PPR;
            roff[k] = (R & 16) + tlb_rho(R & 15);
            soff[k] = 2 * (sp ^ tlb_sigma(R & 15)) * 8;
        }
    }
    auto issue = [&]() {
        const size_t row0 = (blockIdx.x + (size_t)is_next * gridDim.x) * C::ROWS;
        unsigned char* slot = smem + slot_next * C::STAGE_BYTES;
#pragma unroll
        for (int k = 0; k < MYI; ++k) {
            size_t row = row0 + roff[k];
            row = row < m ? row : m - 1;
            __builtin_amdgcn_global_load_lds((wl_gbl_ptr)(Ab + row * (C::N * 8) + soff[k]),
                                             (wl_lds_ptr)(slot + (wave + C::COMPUTE_WAVES * k) * 1024), 16, 0, 2 /* nt */);
        }
        if (wave == 0) {
            size_t row = row0 + (lane >> 1);
            row = row < m ? row : m - 1;
            __builtin_amdgcn_global_load_lds((wl_gbl_ptr)(bb + row * 8 + (lane & 1) * 4),
                                             (wl_lds_ptr)(smem + C::B_OFF + bslot_next * 256), 4, 0, 0);
        }
        is_next = is_next + 1 == (unsigned)S ? 0 : is_next + 1;
        slot_next = (slot_next + 1) % C::NS;
        bslot_next = (bslot_next + 1) % C::NSB;
        ++fissued;
    };
    // own share of stage ff complete (stages ff + 1 .. ff + D issued behind it)
    auto advance = [&]() {
        if constexpr (C::SELF) {
            if (fissued < Ftot) {
                issue();
                if (wave == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::D * (MYI + 1)) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::D * MYI) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
    };
    if constexpr (C::SELF) {
        for (int d = 0; d < C::D && fissued < Ftot; ++d) issue();
        advance();                                              // stage 0
    }

    size_t f = 0;
    for (int ch = 0; ch < nchunks; ++ch) {
        const bool wave_active = ch * C::CHUNK + wave * 16 < P; // wave-uniform
        if (!wave_active) {                                     // nothing to compute: keep the barrier count (and the DMA share)
            for (size_t s = 0; s < S; ++s) {
                __builtin_amdgcn_s_barrier();
                ++f;
                if (f < Ftot) advance();
            }
            continue;
        }
        // lanes past P duplicate point P - 1 (same inputs, same outputs, same addresses): the stores of the sweep
        // need no per-lane predicate and the MFMA + epilogue body stays one basic block
        int pl = ch * C::CHUNK + wave * 16 + fr;
        pl = pl < P ? pl : P - 1;
        double xf[NK];
#pragma unroll
        for (int s = 0; s < NK; ++s) xf[s] = X[(size_t)pl * C::N + 8 * (s >> 1) + 2 * fq + (s & 1)];
        double* yp = DIFF ? Y + (pl >> 1) : (RM ? Y + pl : Y + (size_t)pl * m);
        const size_t ldr = DIFF ? (size_t)(P >> 1) : (RM ? (size_t)P : 1);   // distance between consecutive rows of one point

        // TILES == 2: acc0 / acc1 are the two row tiles of the stage; TILES == 1: the even / odd column pairs of the
        // one tile (two independent chains either way), summed into acc0 at the end
        auto mfma_stage = [&](size_t ff, Acc& acc0, Acc& acc1) {
            const unsigned char* slot = smem + (ff % C::NS) * C::STAGE_BYTES;
            acc0 = Acc{0, 0, 0, 0};
            acc1 = Acc{0, 0, 0, 0};
            if constexpr (C::TILES == 2) {
#pragma unroll
                for (int j = 0; j < NK / 2; ++j) {
                    const int off = laddr[j & 3] + (j >> 2) * 256;  // (4 j & ~15) * 16 bytes
                    const double2 a0 = *reinterpret_cast<const double2*>(slot + off);
                    const double2 a1 = *reinterpret_cast<const double2*>(slot + off + 16 * C::N * 8);
                    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, xf[2 * j], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, xf[2 * j], acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, xf[2 * j + 1], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, xf[2 * j + 1], acc1, 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int j = 0; j < NK / 2; j += 2) {
                    const double2 a0 = *reinterpret_cast<const double2*>(slot + laddr[j & 3] + (j >> 2) * 256);
                    const double2 a1 = *reinterpret_cast<const double2*>(slot + laddr[(j + 1) & 3] + ((j + 1) >> 2) * 256);
                    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, xf[2 * j], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, xf[2 * j + 2], acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, xf[2 * j + 1], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, xf[2 * j + 3], acc1, 0, 0, 0);
                }
                acc0 += acc1;
            }
        };
        // rows row0 + 2 fq + {0, 1} and row0 + 8 + 2 fq + {0, 1} of one 16-row tile
        auto epilogue_tile = [&](const Acc& acc, size_t row0, const unsigned char* bslot, auto full_tag) {
            constexpr bool FULL = decltype(full_tag)::value;
            const double2 b0 = *reinterpret_cast<const double2*>(bslot + 16 * fq);
            const double2 b1 = *reinterpret_cast<const double2*>(bslot + 64 + 16 * fq);
            const double y0 = dtanh(acc[0]) - b0.x, y1 = dtanh(acc[1]) - b0.y;
            const double y2 = dtanh(acc[2]) - b1.x, y3 = dtanh(acc[3]) - b1.y;
            const size_t ra = row0 + 2 * fq, rb = row0 + 8 + 2 * fq;
            if constexpr (DIFF) {
                const double d0 = y0 - lane_pair_swap(y0), d1 = y1 - lane_pair_swap(y1);     // f(x + h e_j) - f(x - h e_j), LS:1041 + 1045
                const double d2 = y2 - lane_pair_swap(y2), d3 = y3 - lane_pair_swap(y3);
                if ((fr & 1) == 0) {
                    if (FULL || ra < m) yp[ra * ldr] = d0;
                    if (FULL || ra + 1 < m) yp[(ra + 1) * ldr] = d1;
                    if (FULL || rb < m) yp[rb * ldr] = d2;
                    if (FULL || rb + 1 < m) yp[(rb + 1) * ldr] = d3;
                }
            } else if constexpr (RM) {
                if (FULL || ra < m) yp[ra * ldr] = y0;
                if (FULL || ra + 1 < m) yp[(ra + 1) * ldr] = y1;
                if (FULL || rb < m) yp[rb * ldr] = y2;
                if (FULL || rb + 1 < m) yp[(rb + 1) * ldr] = y3;
            } else if constexpr (FULL && ALIGNED) {
                *reinterpret_cast<double2*>(yp + ra) = make_double2(y0, y1);
                *reinterpret_cast<double2*>(yp + rb) = make_double2(y2, y3);
            } else if constexpr (FULL) {
                yp[ra] = y0;
                yp[ra + 1] = y1;
                yp[rb] = y2;
                yp[rb + 1] = y3;
            } else {
                if (ra < m) yp[ra] = y0;
                if (ra + 1 < m) yp[ra + 1] = y1;
                if (rb < m) yp[rb] = y2;
                if (rb + 1 < m) yp[rb + 1] = y3;
            }
        };
        auto epilogue = [&](const Acc& e0, const Acc& e1, size_t s, size_t ff, auto full_tag) {
            const size_t row0 = (blockIdx.x + s * (size_t)gridDim.x) * C::ROWS;
            const unsigned char* bs = smem + C::B_OFF + (ff % C::NSB) * 256;
            epilogue_tile(e0, row0, bs, full_tag);
            __builtin_amdgcn_sched_barrier(0);                  // one tile at a time: bounds the live tanh temporaries
            if constexpr (C::TILES == 2) {
                epilogue_tile(e1, row0 + 16, bs + 128, full_tag);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        // The two compute waves of a SIMD (w and w + 4) run out of phase: waves 0..3 do MFMA(s) then epilogue(s),
        // waves 4..7 do epilogue(s - 1) then MFMA(s), so one wave's tanh / store VALU work overlaps the other's
        // MFMA chains without relying on instruction scheduling. Only the last stage of a workgroup can be
        // partial (stages ascend).
        Acc acc0, acc1;
        // (SELF: the wait for this wave's share of the next stage follows the matrix-core chain and precedes the stores)
        if constexpr (GROUP == 0) {
            for (size_t s = 0; s + 1 < S; ++s, ++f) {
                __builtin_amdgcn_s_barrier();                   // stage f is complete in LDS
                mfma_stage(f, acc0, acc1);
                advance();
                epilogue(acc0, acc1, s, f, std::true_type{});
            }
            __builtin_amdgcn_s_barrier();
            mfma_stage(f, acc0, acc1);
            if (f + 1 < Ftot) advance();
            epilogue(acc0, acc1, S - 1, f, std::false_type{});
            ++f;
        } else {
            __builtin_amdgcn_s_barrier();
            mfma_stage(f, acc0, acc1);
            ++f;
            if (f < Ftot) advance();
            for (size_t s = 1; s < S; ++s, ++f) {
                __builtin_amdgcn_s_barrier();
                epilogue(acc0, acc1, s - 1, f - 1, std::true_type{});
                mfma_stage(f, acc0, acc1);
                if (f + 1 < Ftot) advance();
            }
            epilogue(acc0, acc1, S - 1, f - 1, std::false_type{});
        }
    }
}

// ---- difference panel with A read ONCE (p == 2n finite-difference points X = [x + h e_0, x - h e_0, x + h e_1, ...], the
//      contract of mir_lsq_gpu_options.fbRowMajorDiff). The stage loop is the OUTER loop and the point chunks the inner one: a
//      32-row stage of A is DMA'd into LDS once and multiplied with every chunk of points before the ring moves on (the sweep
//      above streams A once per 128-point chunk: 4.1 GB instead of 3.1 at n = 128). What made that impossible for general X
//      is the B operand: 64 VGPRs of X fragments per chunk. Here every row of X is x except in ONE coordinate, so a lane keeps
//      the fragments of x itself (read from rows of X that leave the coordinate alone) plus, per chunk, the one perturbed value
//      and where it goes: the operand of k-step s is a select between the two -- the same numbers the chunked sweep feeds the
//      matrix cores, every product of the dense GEMM is still computed.
template <int NK, int GROUP>
__device__ __forceinline__ void tlb_compute_once(const double* __restrict__ X, double* __restrict__ D, size_t m,
                                                 unsigned char* smem, int lane, int wave, size_t S)
{
    using C = TlbCfg<NK>;
    using Acc = __attribute__((ext_vector_type(4))) double;
    constexpr int N = C::N, P = 2 * C::N;
    constexpr int NCH = (P + C::CHUNK - 1) / C::CHUNK;
    const int fr = lane & 15, fq = lane >> 4;
    const int v = fq ^ tlb_sigma(fr);
    int laddr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) laddr[k] = fr * N * 8 + ((4 * k) ^ v) * 16;

    // fragments of the base point: k-step s multiplies column k = 8 (s >> 1) + 2 fq + (s & 1); rows 2k and 2k + 1 of X perturb it
    double xb[NK];
#pragma unroll
    for (int s = 0; s < NK; ++s) {
        const int k = 8 * (s >> 1) + 2 * fq + (s & 1);
        xb[s] = X[(size_t)((2 * k + 2) % P) * N + k];
    }
    // per chunk: this lane's point, the k-step that carries its perturbed coordinate (if this lane's k-slot has it), the value
    bool act[NCH], hit[NCH];
    int sstar[NCH];
    double xs[NCH];
    double* dp[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        act[c] = c * C::CHUNK + wave * 16 < P;                  // wave-uniform
        int pl = c * C::CHUNK + wave * 16 + fr;
        pl = pl < P ? pl : P - 1;
        const int j = pl >> 1;
        hit[c] = fq == ((j >> 1) & 3);
        sstar[c] = 2 * (j >> 3) + (j & 1);
        xs[c] = X[(size_t)pl * N + j];
        dp[c] = D + j;
    }
    constexpr size_t ldr = N;                                   // D is m x n row-major

    auto mfma_stage = [&](size_t st, auto cc, Acc& acc0, Acc& acc1) {
        constexpr int c = decltype(cc)::value;
        const unsigned char* slot = smem + (st % C::NS) * C::STAGE_BYTES;
        acc0 = Acc{0, 0, 0, 0};
        acc1 = Acc{0, 0, 0, 0};
        auto xop = [&](int s) { return (hit[c] && sstar[c] == s) ? xs[c] : xb[s]; };
        if constexpr (C::TILES == 2) {
#pragma unroll
            for (int j = 0; j < NK / 2; ++j) {
                const int off = laddr[j & 3] + (j >> 2) * 256;
                const double2 a0 = *reinterpret_cast<const double2*>(slot + off);
                const double2 a1 = *reinterpret_cast<const double2*>(slot + off + 16 * N * 8);
                const double x0 = xop(2 * j), x1 = xop(2 * j + 1);
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, x0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, x0, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, x1, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, x1, acc1, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NK / 2; j += 2) {
                const double2 a0 = *reinterpret_cast<const double2*>(slot + laddr[j & 3] + (j >> 2) * 256);
                const double2 a1 = *reinterpret_cast<const double2*>(slot + laddr[(j + 1) & 3] + ((j + 1) >> 2) * 256);
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, xop(2 * j), acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, xop(2 * j + 2), acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, xop(2 * j + 1), acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, xop(2 * j + 3), acc1, 0, 0, 0);
            }
            acc0 += acc1;
        }
    };
    auto epilogue_tile = [&](const Acc& acc, size_t row0, const unsigned char* bslot, double* yp, bool full) {
        const double2 b0 = *reinterpret_cast<const double2*>(bslot + 16 * fq);
        const double2 b1 = *reinterpret_cast<const double2*>(bslot + 64 + 16 * fq);
        const double y0 = dtanh(acc[0]) - b0.x, y1 = dtanh(acc[1]) - b0.y;
        const double y2 = dtanh(acc[2]) - b1.x, y3 = dtanh(acc[3]) - b1.y;
        const double d0 = y0 - lane_pair_swap(y0), d1 = y1 - lane_pair_swap(y1);         // f(x + h e_j) - f(x - h e_j), LS:1041 + 1045
        const double d2 = y2 - lane_pair_swap(y2), d3 = y3 - lane_pair_swap(y3);
        const size_t ra = row0 + 2 * fq, rb = row0 + 8 + 2 * fq;
        if ((fr & 1) == 0) {
            if (full || ra < m) yp[ra * ldr] = d0;
            if (full || ra + 1 < m) yp[(ra + 1) * ldr] = d1;
            if (full || rb < m) yp[rb * ldr] = d2;
            if (full || rb + 1 < m) yp[(rb + 1) * ldr] = d3;
        }
    };
    auto epilogue = [&](const Acc& e0, const Acc& e1, size_t st, auto cc) {
        constexpr int c = decltype(cc)::value;
        const size_t row0 = (blockIdx.x + st * (size_t)gridDim.x) * C::ROWS;
        const unsigned char* bs = smem + C::B_OFF + (st % C::NSB) * 256;
        const bool full = st + 1 < S;                            // only the last stage of a workgroup can be partial
        epilogue_tile(e0, row0, bs, dp[c], full);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (C::TILES == 2) {
            epilogue_tile(e1, row0 + 16, bs + 128, dp[c], full);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // Same phase scheme as tlb_compute over the flat sequence (stage 0, chunk 0), (stage 0, chunk 1), ..., one barrier per STAGE.
    Acc acc0, acc1;
    if constexpr (GROUP == 0) {
        for (size_t st = 0; st < S; ++st) {
            __builtin_amdgcn_s_barrier();                       // stage st is complete in LDS
            wl_static_for<NCH>([&](auto cc) {
                if (act[decltype(cc)::value]) {
                    mfma_stage(st, cc, acc0, acc1);
                    epilogue(acc0, acc1, st, cc);
                }
            });
        }
    } else {
        for (size_t st = 0; st < S; ++st) {
            wl_static_for<NCH>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                if constexpr (c == 0) {
                    __builtin_amdgcn_s_barrier();
                    if (st > 0) {                               // the pending tile is (st - 1, last active chunk)
                        wl_static_for<NCH>([&](auto pp) {
                            constexpr int pc = decltype(pp)::value;
                            constexpr bool last = pc == NCH - 1;
                            if (act[pc] && (last || !act[pc + (last ? 0 : 1)])) epilogue(acc0, acc1, st - 1, pp);
                        });
                    }
                    if (act[0]) mfma_stage(st, cc, acc0, acc1);
                } else {
                    if (act[c]) {                               // act[c] implies act[c - 1]: a wave's chunks fill up from 0
                        epilogue(acc0, acc1, st, std::integral_constant<int, c - 1>{});
                        mfma_stage(st, cc, acc0, acc1);
                    }
                }
            });
        }
        if (S > 0) {
            wl_static_for<NCH>([&](auto pp) {
                constexpr int pc = decltype(pp)::value;
                constexpr bool last = pc == NCH - 1;
                if (act[pc] && (last || !act[pc + (last ? 0 : 1)])) epilogue(acc0, acc1, S - 1, pp);
            });
        }
    }
}

// ---- difference panel by PREFIX FORKING (n = 128, p = 2n finite-difference points, A read once). Points 2 j, 2 j + 1 are x except
//      in coordinate j, and k-step s of the chain multiplies columns 8 (s >> 1) + 2 fq + (s & 1): the 16-point group g (coordinates
//      8 g .. 8 g + 7) meets its own coordinates first at k-step 2 g. Before that every column of its MFMAs has the inputs of the
//      chain of x itself (same A fragment, same B value, same accumulator), and an element of an MFMA result depends only on its
//      own row, column and accumulator: the group's accumulator after 2 g steps IS the base chain's P_2g, bit for bit. So
//        * the two loader waves also run the base chain of one tile each, one stage ahead of the compute waves, and publish
//          P_2, P_4, ..., P_30 through LDS (16 doubles per prefix and tile). The base chain is A times ONE vector, so it runs
//          on v_mfma_f64_4x4x4_4b_f64 (four 4-row blocks, x in 4 columns, 16 cycles of the matrix pipe) and not on the
//          16x16x4 form (x in 16 columns, 64 cycles): the same fused multiply-adds per element, the same bits;
//        * compute wave w owns the two groups of tlb_fork_group(w, .), starts each from its prefix, then runs the group's own
//          k-steps 2 g .. NK - 1 in the order of tlb_compute: 272 16x16x4 MFMAs per tile instead of 512, and 30 short ones.
//          Balance: a group costs 32 - 2 g k-steps per tile, and the loader waves 8, 9 share the SIMDs of waves 0, 4 and
//          1, 5 (waves w and w + 4 share one). Those four waves get 30 k-steps per tile ({2, 15}, {3, 14}, {6, 11}, {7, 10})
//          and the other four 38 ({0, 13}, {1, 12}, {4, 9}, {5, 8});
//        * a stage of A is DMA'd once for all 256 points; the epilogue is tlb_compute's, with the row compares compiled out
//          of every stage but a workgroup's last and the store addresses carried from stage to stage.
//      The structure is never assumed: tlb_fork_vote compares, as bit patterns, every X entry a forked chain takes from the base
//      chain with the base value, and the workgroup runs the dense tlb_compute unless all of them agree.
//      Barriers: the loaders pass B_f once stage f is in LDS, then DMA stage f + D and run the base chain of f; the compute waves
//      compute stage f after B_{f + 1} (its prefixes are written by then). So a stage occupies a ring slot until B_{f + 2} and
//      the DMA of f + D is issued after B_f, not before: D + 2 = NS slots.

// every compute lane checks its two points over the k-steps their chains take from the base chain; true: all equal
template <int NK>
__device__ __forceinline__ bool tlb_fork_vote(const double* __restrict__ X, unsigned char* smem, int lane, int wave)
{
    using C = TlbCfg<NK>;
    constexpr int N = C::N, P = 2 * N;
    volatile int* vote = reinterpret_cast<volatile int*>(smem + C::VOTE_OFF);
    if (threadIdx.x == 0) *vote = 0;
    __syncthreads();
    if (wave < C::COMPUTE_WAVES) {
        const int fr = lane & 15, fq = lane >> 4;
        const int s0 = 2 * tlb_fork_group(wave, 0), s1 = 2 * tlb_fork_group(wave, 1);   // its groups (tlb_fork_compute) fork at s0, s1
        const unsigned long long* xr = reinterpret_cast<const unsigned long long*>(X);
        const unsigned long long* x0 = xr + (size_t)(8 * s0 + fr) * N;         // point 16 g + fr
        const unsigned long long* x1 = xr + (size_t)(8 * s1 + fr) * N;
        bool bad = false;
#pragma unroll
        for (int s = 0; s < NK - 2; ++s) {
            const int k = 8 * (s >> 1) + 2 * fq + (s & 1);
            const unsigned long long xb = xr[(size_t)((2 * k + 2) % P) * N + k];  // the base value, as tlb_compute_once reads it
            const unsigned long long a = x0[k], c = x1[k];
            bad |= (s < s0) & (a != xb);
            bad |= (s < s1) & (c != xb);
        }
        if (bad) *vote = 1;
    }
    __syncthreads();
    return *vote == 0;
}

template <int NK, int LOADER>
__device__ __forceinline__ void tlb_fork_loader(const double* __restrict__ A, const double* __restrict__ b,
                                                const double* __restrict__ X, size_t m, unsigned char* smem, int lane, size_t S)
{
    using C = TlbCfg<NK>;
    constexpr int N = C::N, P = 2 * N;
    constexpr int OPS = C::IPS / 2 + (LOADER == 1 ? 1 : 0);
    const int fr = lane & 15, fq = lane >> 4;
    const int v = fq ^ tlb_sigma(fr);
    int laddr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) laddr[k] = LOADER * 16 * N * 8 + fr * N * 8 + ((4 * k) ^ v) * 16;   // tile LOADER of a stage
    double xb[2 * C::NPRE];
#pragma unroll
    for (int s = 0; s < 2 * C::NPRE; ++s) {
        const int k = 8 * (s >> 1) + 2 * fq + (s & 1);
        xb[s] = X[(size_t)((2 * k + 2) % P) * N + k];
    }
    auto issue = [&](size_t f) { tlb_issue<NK, LOADER>(A, b, m, smem, lane, S, f); };
    for (size_t f = 0; f < S && f < (size_t)C::D; ++f) issue(f);
    for (size_t f = 0; f < S; ++f) {
        if (f + 1 < S) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(OPS) : "memory");   // stage f + 1 may still be in flight
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                       // B_f: stage f is in LDS; stage f - 2 has no readers left
        asm volatile("" ::: "memory");
        if (f + C::D < S) issue(f + C::D);
        // base chain of tile LOADER of stage f on v_mfma_f64_4x4x4_4b_f64: four blocks of 4 rows x 4 columns, 16 cycles of the
        // matrix pipe instead of the 64 of the 16x16x4 form, whose 16 columns would all hold x. Lane i + 4 b + 16 k holds A[4 b + i][k]
        // -- row fr, k = fq: the 16x16x4 A operand, so the same LDS reads -- lane j + 4 b + 16 k holds B[k][j] = x[k], and the
        // result lane j + 4 b + 16 i holds row 4 b + i. Each element is the same sequence of four fused multiply-adds as in
        // the 16x16x4 form: every prefix is bitwise equal (scripts/probes/f64_mfma_4x4_probe.hip). After k-steps 2 j + 1 the
        // lanes of column j = 0 store P_{2 j + 2}: row 4 b + i = D row fq + 4 r with fq = i, r = b.
        const unsigned char* slot = smem + (f % C::NS) * C::STAGE_BYTES;
        double* pre = reinterpret_cast<double*>(smem + C::PRE_OFF + (f & 1) * C::PRE_STAGE) + LOADER * C::NPRE * 16 + 4 * fq + (fr >> 2);
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < C::NPRE; ++j) {
            const double2 a = *reinterpret_cast<const double2*>(slot + laddr[j & 3] + (j >> 2) * 256);
            acc = __builtin_amdgcn_mfma_f64_4x4x4f64(a.x, xb[2 * j], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_4x4x4f64(a.y, xb[2 * j + 1], acc, 0, 0, 0);
            if ((fr & 3) == 0) pre[16 * j] = acc;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // the prefixes are in LDS before the next barrier
    }
    __builtin_amdgcn_s_barrier();                           // B_S: the prefixes of the last stage
}

template <int NK, int W, bool BASE = false>
__device__ __forceinline__ void tlb_fork_compute(const double* __restrict__ X, double* __restrict__ D, size_t m,
                                                 unsigned char* smem, int lane, size_t S)
{
    using C = TlbCfg<NK>;
    using Acc = __attribute__((ext_vector_type(4))) double;
    constexpr int N = C::N;
    constexpr int GA = tlb_fork_group(W, 0), GC = tlb_fork_group(W, 1);   // this wave's two groups (see the balance note above)
    constexpr int SA = 2 * GA, SC = 2 * GC;                 // the k-step where each forks off the base chain
    constexpr int GROUP = W < C::COMPUTE_WAVES / 2 ? 0 : 1; // waves w and w + 4 share a SIMD: run them out of phase
    const int fr = lane & 15, fq = lane >> 4;
    const int v = fq ^ tlb_sigma(fr);
    int laddr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) laddr[k] = fr * N * 8 + ((4 * k) ^ v) * 16;
    const int pa = 16 * GA + fr, pc = 16 * GC + fr;
    double xa[NK - SA], xc[NK - SC];
#pragma unroll
    for (int s = SA; s < NK; ++s) xa[s - SA] = X[(size_t)pa * N + 8 * (s >> 1) + 2 * fq + (s & 1)];
#pragma unroll
    for (int s = SC; s < NK; ++s) xc[s - SC] = X[(size_t)pc * N + 8 * (s >> 1) + 2 * fq + (s & 1)];
    constexpr size_t ldr = N;                               // D is m x n row-major
    // Where this lane stores: sb is the pending stage's first row, the same for the whole wave (scalar registers), and voff
    // the lane's own byte offset in it: row 2 fq, group GA's column. Group GC's column is DC doubles further, and the
    // lane's other rows lie 1, 8, 9, 16, ... rows below: compile-time offsets. sb advances by one stage of the grid after
    // every epilogue (the epilogues run in stage order), so a stage's sixteen store addresses cost a few 64-bit adds and
    // immediate offsets, not a shift and a shift-add per store.
    constexpr int DC = 8 * (GC - GA);
    const unsigned voff = (unsigned)(((pa >> 1) + 2 * fq * ldr) * 8);
    unsigned char* sb = reinterpret_cast<unsigned char*>(D + (size_t)blockIdx.x * C::ROWS * ldr);
    const size_t stage_step = (size_t)gridDim.x * C::ROWS * ldr * 8;

    // acc[0], acc[1]: group GA, tiles 0 and 1; acc[2], acc[3]: group GC
    auto mfma_stage = [&](size_t f, Acc (&acc)[4]) {
        const unsigned char* slot = smem + (f % C::NS) * C::STAGE_BYTES;
        const double* pre = reinterpret_cast<const double*>(smem + C::PRE_OFF + (f & 1) * C::PRE_STAGE) + 4 * fq;
        auto prefix = [&](int t, int s) {                   // P_s of tile t, this lane's rows fq + 4 r
            if (s == 0) return Acc{0.0, 0.0, 0.0, 0.0};
            const double* p = pre + (t * C::NPRE + s / 2 - 1) * 16;
            const double2 lo = *reinterpret_cast<const double2*>(p), hi = *reinterpret_cast<const double2*>(p + 2);
            return Acc{lo.x, lo.y, hi.x, hi.y};
        };
        acc[0] = prefix(0, SA);
        acc[1] = prefix(1, SA);
        acc[2] = prefix(0, SC);
        acc[3] = prefix(1, SC);
        wl_static_for<NK / 2 - GA>([&](auto jj) {
            constexpr int j = GA + decltype(jj)::value;
            const int off = laddr[j & 3] + (j >> 2) * 256;
            const double2 a0 = *reinterpret_cast<const double2*>(slot + off);
            const double2 a1 = *reinterpret_cast<const double2*>(slot + off + 16 * N * 8);
            acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, xa[2 * j - SA], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, xa[2 * j - SA], acc[1], 0, 0, 0);
            if constexpr (j >= GC) {
                acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, xc[2 * j - SC], acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, xc[2 * j - SC], acc[3], 0, 0, 0);
            }
            acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, xa[2 * j + 1 - SA], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, xa[2 * j + 1 - SA], acc[1], 0, 0, 0);
            if constexpr (j >= GC) {
                acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, xc[2 * j + 1 - SC], acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, xc[2 * j + 1 - SC], acc[3], 0, 0, 0);
            }
        });
    };
    // yb + voff: row ra = 2 fq of the tile in the group's column; the lane's rows are ra, ra + 1, ra + 8, ra + 9
    auto epilogue_tile = [&](const Acc& acc, unsigned char* yb, size_t ra, const unsigned char* bslot, auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        const double2 b0 = *reinterpret_cast<const double2*>(bslot + 16 * fq);
        const double2 b1 = *reinterpret_cast<const double2*>(bslot + 64 + 16 * fq);
        const double y0 = dtanh(acc[0]) - b0.x, y1 = dtanh(acc[1]) - b0.y;
        const double y2 = dtanh(acc[2]) - b1.x, y3 = dtanh(acc[3]) - b1.y;
        const double d0 = y0 - lane_pair_swap(y0), d1 = y1 - lane_pair_swap(y1);         // f(x + h e_j) - f(x - h e_j), LS:1041 + 1045
        const double d2 = y2 - lane_pair_swap(y2), d3 = y3 - lane_pair_swap(y3);
        double* const yp = reinterpret_cast<double*>(yb + voff);
        if ((fr & 1) == 0) {
            if (FULL || ra < m) yp[0] = d0;
            if (FULL || ra + 1 < m) yp[ldr] = d1;
            if (FULL || ra + 8 < m) yp[8 * ldr] = d2;
            if (FULL || ra + 9 < m) yp[9 * ldr] = d3;
        }
    };
    // the pending stage f; FULL: all its 32 rows exist (only the last stage of a workgroup can be partial), no row is compared
    auto epilogue = [&](const Acc (&acc)[4], size_t f, auto full_tag) {
        const size_t ra = (blockIdx.x + f * (size_t)gridDim.x) * C::ROWS + 2 * fq;
        const unsigned char* bs = smem + C::B_OFF + (f % C::NSB) * 256;
        epilogue_tile(acc[0], sb, ra, bs, full_tag);
        __builtin_amdgcn_sched_barrier(0);                  // one tile at a time: bounds the live tanh temporaries
        epilogue_tile(acc[1], sb + 16 * ldr * 8, ra + 16, bs + 128, full_tag);
        __builtin_amdgcn_sched_barrier(0);
        epilogue_tile(acc[2], sb + DC * 8, ra, bs, full_tag);
        __builtin_amdgcn_sched_barrier(0);
        epilogue_tile(acc[3], sb + (DC + 16 * ldr) * 8, ra + 16, bs + 128, full_tag);
        __builtin_amdgcn_sched_barrier(0);
        sb += stage_step;
    };
    auto barrier = [] {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    // BASE: the extra point of a p = 2n + 1 call, four rows of stage f per share (the stage's slot is held until B_{f + 2}).
    // Waves 2 and 3 -- 38 k-steps per tile and the epilogue straight behind the chains: 168 registers without this -- take none:
    // with a share they kept a dozen values in scratch memory, reloaded every stage behind the epilogue's stores. Their shares
    // go to waves 6 and 7, which sit on the same two SIMDs, so every SIMD still carries eight rows per stage.
    constexpr int BASE_SHARES = !BASE || W == 2 || W == 3 ? 0 : W >= 6 ? 2 : 1;
    [[maybe_unused]] auto base_rows = [&](size_t f) {
        wl_static_for<BASE_SHARES>([&](auto hh) {
            tlb_base_rows<NK>(smem + (f % C::NS) * C::STAGE_BYTES, smem + C::B_OFF + (f % C::NSB) * 256, smem, D + m * ldr,
                              (blockIdx.x + f * (size_t)gridDim.x) * C::ROWS, m, W - 4 * decltype(hh)::value);
            __builtin_amdgcn_sched_barrier(0);              // between two stages' accumulators, mixed with neither: no registers to spare
        });
    };
    Acc acc[4];
    barrier();                                              // B_0
    if constexpr (GROUP == 0) {
        for (size_t f = 0; f < S; ++f) {
            barrier();                                      // B_{f + 1}: stage f and its prefixes are in LDS
            base_rows(f);
            mfma_stage(f, acc);
            if (f + 1 < S) epilogue(acc, f, std::true_type{});
            else epilogue(acc, f, std::false_type{});
        }
    } else {
        barrier();
        base_rows(0);
        mfma_stage(0, acc);
        for (size_t f = 1; f < S; ++f) {
            barrier();
            epilogue(acc, f - 1, std::true_type{});
            base_rows(f);
            mfma_stage(f, acc);
        }
        epilogue(acc, S - 1, std::false_type{});
    }
}

// The same point when X fails tlb_fork_vote and the workgroup has run the chunked sweep (tests and foreign X only: the sweep's
// compute waves have neither vector nor scalar registers to spare for tlb_base_rows): behind the sweep, every wave takes its
// share of the workgroup's stages once more from memory -- the one-point kernel's loads, lanes and arithmetic.
template <int NK>
__device__ __forceinline__ void tlb_base_sweep(const double* __restrict__ A, const double* __restrict__ b, const double* __restrict__ x,
                                               double* __restrict__ ybase, size_t m, int wave, size_t S)
{
    using C = TlbCfg<NK>;
    static_assert(C::N == 128, "four column pairs a lane");
    const int lane = tlb_lane_now();                        // (nothing of this is alive during the sweeps before it)
    const int q = lane >> 4, p = lane & 15;
    double x0[4], x1[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double2 t = *reinterpret_cast<const double2*>(x + 32 * c + 2 * p);
        x0[c] = t.x; x1[c] = t.y;
    }
    for (size_t k = wave; k < S; k += C::THREADS / 64) {
        const size_t row0 = (blockIdx.x + k * (size_t)gridDim.x) * C::ROWS;
        for (int g = 0; g < C::ROWS / 4; ++g) {
            const size_t row = row0 + 4 * g + q, rc = row < m ? row : m - 1;
            double v0[4], v1[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double2 t = *reinterpret_cast<const double2*>(A + rc * C::N + 32 * c + 2 * p);
                v0[c] = t.x; v1[c] = t.y;
            }
            const double s = sum16(tanh_linear_row_sum<double, 4>(v0, v1, x0, x1));
            const double t = dtanh(s);
            if (p == 0 && row < m) ybase[row] = t - b[rc];
        }
    }
}

template <int NK, bool RM = false, bool DIFF = false, bool BASE = false>
__global__ __launch_bounds__(TlbCfg<NK>::THREADS) void k_tanh_linear_batched_dma(const double* __restrict__ A,
                                                                                  const double* __restrict__ b,
                                                                                  const double* __restrict__ X,
                                                                                  double* __restrict__ Y, size_t m, int P,
                                                                                  int mode)
{
    using C = TlbCfg<NK>;
    extern __shared__ __attribute__((aligned(16))) unsigned char tlb_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t Stot = (m + C::ROWS - 1) / C::ROWS;
    const size_t S = blockIdx.x < Stot ? (Stot - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;   // stages blockIdx.x + k grid
    const int nchunks = (P + C::CHUNK - 1) / C::CHUNK;
    // the finite-difference points of fbRowMajorDiff, on request: A is read once (2.1 instead of 3.1 GB per call at n = 128,
    // and 3 % SLOWER: the kernel is MFMA-bound and the operand selects are extra VALU work -- not the default)
    // (n = 256: six chunks of per-chunk state next to 128 VGPRs of fragments spill -- measured 2x slower; not offered there)
    // mode: 0 = the chunked sweep (tlb_compute), 1 = read A once (tlb_compute_once), 2 = prefix forking (n = 128) when X passes
    // tlb_fork_vote, else the chunked sweep
    const bool once = DIFF && mode == 1 && NK <= 32 && P == 2 * C::N;
    const size_t F = once ? S : S * (size_t)nchunks;            // flat (chunk, stage) sequence: the ring never drains
    if (S == 0) return;
    if constexpr (BASE) {                                   // (launched with P = 2n and mode 0 or 2 only) the extra point: row P of X
        static_assert(DIFF && C::FORK, "the extra point rides on the n = 128 difference panel");
        if (threadIdx.x < C::N) reinterpret_cast<double*>(tlb_smem + C::BASE_OFF)[threadIdx.x] = X[(size_t)P * C::N + threadIdx.x];
        __syncthreads();
    }
    if constexpr (DIFF && C::FORK) {
        if (mode == 2 && P == 2 * C::N && tlb_fork_vote<NK>(X, tlb_smem, lane, wave)) {       // (workgroup-uniform)
            if (wave == C::COMPUTE_WAVES) tlb_fork_loader<NK, 0>(A, b, X, m, tlb_smem, lane, S);
            else if (wave == C::COMPUTE_WAVES + 1) tlb_fork_loader<NK, 1>(A, b, X, m, tlb_smem, lane, S);
            else wl_static_for<C::COMPUTE_WAVES>([&](auto ww) {
                if (wave == decltype(ww)::value) tlb_fork_compute<NK, decltype(ww)::value, BASE>(X, Y, m, tlb_smem, lane, S);
            });
            return;
        }
    }
    if (!C::SELF && wave == C::COMPUTE_WAVES) tlb_loader<NK, 0>(A, b, m, tlb_smem, lane, S, F);
    else if (!C::SELF && wave == C::COMPUTE_WAVES + 1) tlb_loader<NK, 1>(A, b, m, tlb_smem, lane, S, F);
    else if (DIFF && once) {
        if constexpr (DIFF) {
            if (wave < 4) tlb_compute_once<NK, 0>(X, Y, m, tlb_smem, lane, wave, S);     // waves w and w + 4 share a SIMD
            else tlb_compute_once<NK, 1>(X, Y, m, tlb_smem, lane, wave, S);
        }
    } else {
        if constexpr (RM) {
            if (wave < 4) tlb_compute<NK, false, 0, true, DIFF>(A, b, X, Y, m, P, tlb_smem, lane, wave, S, nchunks);
            else tlb_compute<NK, false, 1, true, DIFF>(A, b, X, Y, m, P, tlb_smem, lane, wave, S, nchunks);
        } else {
            const bool aligned = ((m & 1) == 0) && ((reinterpret_cast<uintptr_t>(Y) & 15) == 0);
            if (wave < 4) {
                if (aligned) tlb_compute<NK, true, 0>(A, b, X, Y, m, P, tlb_smem, lane, wave, S, nchunks);
                else tlb_compute<NK, false, 0>(A, b, X, Y, m, P, tlb_smem, lane, wave, S, nchunks);
            } else {
                if (aligned) tlb_compute<NK, true, 1>(A, b, X, Y, m, P, tlb_smem, lane, wave, S, nchunks);
                else tlb_compute<NK, false, 1>(A, b, X, Y, m, P, tlb_smem, lane, wave, S, nchunks);
            }
        }
    }
    if constexpr (BASE) tlb_base_sweep<NK>(A, b, X + (size_t)P * C::N, Y + m * (size_t)C::N, m, wave, S);
}

template <int NK, bool RM = false, bool DIFF = false, bool BASE = false>
bool launch_tlb_dma(const double* A, const double* b, const double* X, double* Y, size_t m, int P, hipStream_t s, int mode = 0)
{
    using C = TlbCfg<NK>;
    constexpr int lds = BASE ? C::BASE_LDS_BYTES : DIFF && C::FORK ? C::FORK_LDS_BYTES : C::LDS_BYTES;
    static bool attr_ok = [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(k_tanh_linear_batched_dma<NK, RM, DIFF, BASE>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
    }();
    if (!attr_ok) return false;
    const size_t Stot = (m + C::ROWS - 1) / C::ROWS;
    const unsigned grid = (unsigned)(Stot < 256 ? Stot : 256);
    hipLaunchKernelGGL((k_tanh_linear_batched_dma<NK, RM, DIFF, BASE>), dim3(grid), dim3(C::THREADS), lds, s, A, b, X, Y, m, P, mode);
    return true;
}

// row-major output for shapes the DMA kernel does not cover: one thread per (row, point), plain dot product
__global__ __launch_bounds__(256) void k_tanh_linear_batched_rm_generic(const double* __restrict__ A, const double* __restrict__ b,
                                                                        const double* __restrict__ X, double* __restrict__ Y,
                                                                        size_t m, int n, int P)
{
    const size_t total = m * (size_t)P;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t i = e / P;
        const int k = (int)(e % P);
        const double* a = A + i * (size_t)n;
        const double* x = X + (size_t)k * n;
        double s0 = 0;
        for (int j = 0; j < n; ++j) s0 += a[j] * x[j];
        Y[e] = dtanh(s0) - b[i];
    }
}

// difference panel for shapes the DMA kernel does not cover: one thread per (row, column), two dot products
__global__ __launch_bounds__(256) void k_tanh_linear_batched_diff_generic(const double* __restrict__ A, const double* __restrict__ b,
                                                                          const double* __restrict__ X, double* __restrict__ D,
                                                                          size_t m, int n, int P)
{
    const int nc = P / 2;
    const size_t total = m * (size_t)nc;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t i = e / nc;
        const int j = (int)(e % nc);
        const double* a = A + i * (size_t)n;
        const double* xp = X + (size_t)(2 * j) * n;
        const double* xm = xp + n;
        double sp = 0, sm = 0;
        for (int k = 0; k < n; ++k) { sp += a[k] * xp[k]; sm += a[k] * xm[k]; }
        const double yp = dtanh(sp) - b[i], ym = dtanh(sm) - b[i];
        D[e] = yp - ym;
    }
}

// ---- any n above the LDS-DMA shapes (n > 256, n % 8 == 0): the same GEMM on the matrix cores with both operands read straight
//      from memory (A streamed once per workgroup: its four waves share a 16-row tile through L1 / L2; X, a few MB, lives in L2).
//      A wave owns 16 rows x 64 points (four accumulators reuse each A fragment); the K index is permuted as in the LDS-DMA kernel
//      so that one 16-byte load feeds two k-steps: lane (fr, fq) reads columns 8 j + 2 fq, + 1 of its row / of its point.
//      (Before: one thread per (row, point) with a scalar dot product, 236 ms for the 1024 points of an n = 512 refresh at
//      m = 250 000 -- 1.1 TFLOP/s; the solver's own work at that shape is 20 ms.)
// OUT: 0 = Y m x P row-major, 1 = the m x P/2 row-major DIFFERENCE panel, 2 = Y point-major (Y[k m + i])
template <int OUT>
__global__ __launch_bounds__(256) void k_tanh_linear_batched_wide(const double* __restrict__ A, const double* __restrict__ b,
                                                                    const double* __restrict__ X, double* __restrict__ Y,
                                                                    size_t m, int n, int P)
{
    // A wave owns RT = 4 row tiles x 4 point tiles (64 rows x 64 points, 128 accumulator registers): per pair of k-steps 4 + 4
    // sixteen-byte loads feed 32 MFMAs. With one row tile (1 + 4 loads for 8 MFMAs) the kernel ran at the CU's vector-memory address
    // rate and re-read its points' 256 KB of X from L2 for every 16 rows: the 1024 points of an n = 512 refresh at m = 250 000 took
    // 8.8 ms (30 TFLOP/s); two row tiles 7.4, four 6.7 (39 TFLOP/s, one wave a SIMD). The next step would be X and A through LDS.
    constexpr int RT = 4;
    using Acc = __attribute__((ext_vector_type(4))) double;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const size_t ntiles = (m + 16 * RT - 1) / (16 * RT);
    const int ngroups = (P + 63) / 64;
    const int npairs = n / 8;
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const double2* __restrict__ ap[RT];
        double bv[RT][4];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const size_t r0 = (t * RT + rt) * 16;
            const size_t arow = r0 + fr < m ? r0 + fr : m - 1;
            ap[rt] = reinterpret_cast<const double2*>(A + arow * (size_t)n) + fq;
#pragma unroll
            for (int r = 0; r < 4; ++r) { const size_t row = r0 + fq + 4 * r; bv[rt][r] = b[row < m ? row : m - 1]; }
        }
        for (int g = wave; g < ngroups; g += 4) {
            const double2* __restrict__ xp[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                int pt = 64 * g + 16 * u + fr;
                pt = pt < P ? pt : P - 1;
                xp[u] = reinterpret_cast<const double2*>(X + (size_t)pt * n) + fq;
            }
            Acc acc[RT][4];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[rt][u] = Acc{0, 0, 0, 0};
#pragma unroll 2
            for (int j = 0; j < npairs; ++j) {
                double2 a[RT], x[4];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) a[rt] = ap[rt][4 * j];
#pragma unroll
                for (int u = 0; u < 4; ++u) x[u] = xp[u][4 * j];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        acc[rt][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rt].x, x[u].x, acc[rt][u], 0, 0, 0);
                        acc[rt][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rt].y, x[u].y, acc[rt][u], 0, 0, 0);
                    }
            }
            // D: column = lane & 15 = point, rows fq + 4 r
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int pt = 64 * g + 16 * u + fr;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const size_t row = (t * RT + rt) * 16 + fq + 4 * r;
                        const double y = dtanh(acc[rt][u][r]) - bv[rt][r];
                        if constexpr (OUT == 1) {
                            const double d = y - lane_pair_swap(y);              // f(x + h e_j) - f(x - h e_j): points 2 j, 2 j + 1 are adjacent lanes
                            if ((fr & 1) == 0 && pt < P && row < m) Y[row * (size_t)(P >> 1) + (pt >> 1)] = d;
                        } else if constexpr (OUT == 0) {
                            if (pt < P && row < m) Y[row * (size_t)P + pt] = y;
                        } else {
                            if (pt < P && row < m) Y[(size_t)pt * m + row] = y;
                        }
                    }
                }
        }
    }
}

}  // namespace

// The launchers take the class tl_class (workloads_gemm.h) chose: nothing here decides a shape.
bool launch_tlb_dma_class(const TlClass& c, const double* A, const double* b, const double* X, double* Y, size_t m, int P, hipStream_t s,
                          int read_a_once, bool dense)
{
    if (c.flags & TL_DIFF) {                               // whole 16-point MFMA tiles: no clamped lanes, whose pairs would store zeros
        const int mode = read_a_once ? 1 : dense ? 0 : 2;
        // the extra point of a p = 2n + 1 call rides on the n = 128 kernel (forked or dense; not on the read-A-once experiment)
        if (c.flags & TL_BASE) return launch_tlb_dma<32, true, true, true>(A, b, X, Y, m, P, s, mode);
        switch (c.width) {
        case 64: return launch_tlb_dma<64, true, true>(A, b, X, Y, m, P, s, mode);
        case 32: return launch_tlb_dma<32, true, true>(A, b, X, Y, m, P, s, mode);
        case 16: return launch_tlb_dma<16, true, true>(A, b, X, Y, m, P, s, mode);
        default: return launch_tlb_dma<8, true, true>(A, b, X, Y, m, P, s, mode);
        }
    }
    if (c.flags & TL_RM) {
        switch (c.width) {
        case 64: return launch_tlb_dma<64, true>(A, b, X, Y, m, P, s);
        case 32: return launch_tlb_dma<32, true>(A, b, X, Y, m, P, s);
        case 16: return launch_tlb_dma<16, true>(A, b, X, Y, m, P, s);
        default: return launch_tlb_dma<8, true>(A, b, X, Y, m, P, s);
        }
    }
    switch (c.width) {
    case 64: return launch_tlb_dma<64>(A, b, X, Y, m, P, s);
    case 32: return launch_tlb_dma<32>(A, b, X, Y, m, P, s);
    case 16: return launch_tlb_dma<16>(A, b, X, Y, m, P, s);
    default: return launch_tlb_dma<8>(A, b, X, Y, m, P, s);
    }
}

void launch_tanh_linear_gemm_class(const TlClass& c, const double* A, const double* b, const double* X, double* Y, size_t m, int n, int P,
                                   hipStream_t s)
{
    if (c.family == TL_WIDE) {
        const size_t nt = (m + 63) / 64;
        const dim3 grid((unsigned)(nt < 256 * 8 ? nt : 256 * 8));
        if (c.width == 0) hipLaunchKernelGGL(k_tanh_linear_batched_wide<0>, grid, dim3(256), 0, s, A, b, X, Y, m, n, P);
        else if (c.width == 1) hipLaunchKernelGGL(k_tanh_linear_batched_wide<1>, grid, dim3(256), 0, s, A, b, X, Y, m, n, P);
        else hipLaunchKernelGGL(k_tanh_linear_batched_wide<2>, grid, dim3(256), 0, s, A, b, X, Y, m, n, P);
    } else if (c.family == TL_GENERIC_DIFF) {
        size_t blocks = (m * (size_t)(P / 2) + 255) / 256;
        if (blocks > 256 * 16) blocks = 256 * 16;
        hipLaunchKernelGGL(k_tanh_linear_batched_diff_generic, dim3((unsigned)(blocks ? blocks : 1)), dim3(256), 0, s, A, b, X, Y, m, n, P);
    } else if (c.family == TL_GENERIC_RM) {
        size_t blocks = (m * (size_t)P + 255) / 256;
        if (blocks > 256 * 16) blocks = 256 * 16;
        hipLaunchKernelGGL(k_tanh_linear_batched_rm_generic, dim3((unsigned)(blocks ? blocks : 1)), dim3(256), 0, s, A, b, X, Y, m, n, P);
    } else {                                               // TL_MFMA
        const size_t ntiles = (m + 15) / 16;
        const unsigned grid = (unsigned)(ntiles < 256 ? ntiles : 256);
        if (c.width == 4) hipLaunchKernelGGL(k_tanh_linear_batched<4>, dim3(grid), dim3(1024), 0, s, A, b, X, Y, m, n, P);
        else if (c.width == 8) hipLaunchKernelGGL(k_tanh_linear_batched<8>, dim3(grid), dim3(1024), 0, s, A, b, X, Y, m, n, P);
        else if (c.width == 16) hipLaunchKernelGGL(k_tanh_linear_batched<16>, dim3(grid), dim3(1024), 0, s, A, b, X, Y, m, n, P);
        else hipLaunchKernelGGL(k_tanh_linear_batched<32>, dim3(grid), dim3(1024), 0, s, A, b, X, Y, m, n, P);
    }
}
