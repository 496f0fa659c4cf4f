// f64_mfma_4x4_probe.hip -- can v_mfma_f64_4x4x4_4b_f64 (16 cycles) stand in for v_mfma_f64_16x16x4_f64 (64 cycles) on the
// base chain of the forked difference-panel GEMM (csrc/workloads_gemm.hip, tlb_fork_loader)? The base chain multiplies a
// 16-row tile of A with ONE vector x; the 16x16x4 form repeats x in all 16 columns. Three questions:
//   1. layout: which lane holds which element of A, B and D in the four-block 4x4x4 form. Assumed (and checked over all
//      64 x 64 one-hot operand pairs):  A[i][k] of block b in lane i + 4 b + 16 k,  B[k][j] of block b in lane j + 4 b + 16 k,
//      D[i][j] of block b in lane j + 4 b + 16 i.  With rows = 4 b + i that is the A layout of the 16x16x4 form (row = lane & 15,
//      k = lane >> 4): the same LDS reads feed both.
//   2. bits: a chain of 32 k-steps over random A and x, every prefix P_1 .. P_32 compared as bit patterns: 16x16x4 against 4x4x4
//      and against a plain fma chain in the order k = 0, 1, 2, 3 within a k-step.
//   3. time: cycles per MFMA of one dependent chain of each form (one wave on its SIMD, nothing beside it).
// Build + run on the GPU box:  hipcc --offload-arch=gfx950 -O3 -o /tmp/f64_mfma_4x4 scripts/probes/f64_mfma_4x4_probe.hip && /tmp/f64_mfma_4x4
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <vector>

typedef __attribute__((ext_vector_type(4))) double Acc;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

// 1. out[la * 64 + lb] = ballot of the lanes whose D is nonzero when only lane la holds A = 1 and only lane lb holds B = 1
__global__ __launch_bounds__(64) void k_layout(unsigned long long* out)
{
    const int lane = threadIdx.x;
    for (int la = 0; la < 64; ++la)
        for (int lb = 0; lb < 64; ++lb) {
            const double a = lane == la ? 1.0 : 0.0, b = lane == lb ? 1.0 : 0.0;
            const double d = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, 0.0, 0, 0, 0);
            const unsigned long long m = __ballot(d != 0.0);
            if (lane == 0) out[la * 64 + lb] = m;
        }
}

// 2. one wave per tile: A is tiles x 16 x 128 row-major, x is tiles x 128; P is tiles x 3 x 32 x 16 (form, k-step, row)
__global__ __launch_bounds__(64) void k_bits(const double* __restrict__ A, const double* __restrict__ X, double* __restrict__ P)
{
    const int lane = threadIdx.x, fr = lane & 15, fq = lane >> 4;
    const double* a = A + (size_t)blockIdx.x * 16 * 128 + fr * 128;
    const double* x = X + (size_t)blockIdx.x * 128;
    double* p = P + (size_t)blockIdx.x * 3 * 32 * 16;
    Acc big = {0.0, 0.0, 0.0, 0.0};
    double small = 0.0, chain = 0.0;
    for (int s = 0; s < 32; ++s) {
        big = __builtin_amdgcn_mfma_f64_16x16x4f64(a[4 * s + fq], x[4 * s + fq], big, 0, 0, 0);
        small = __builtin_amdgcn_mfma_f64_4x4x4f64(a[4 * s + fq], x[4 * s + fq], small, 0, 0, 0);
        for (int k = 0; k < 4; ++k) chain = fma(a[4 * s + k], x[4 * s + k], chain);        // (every fq group computes row fr)
        if (fr == 0)                                                                        // D of 16x16x4: column 0, rows fq + 4 r
            for (int r = 0; r < 4; ++r) p[(0 * 32 + s) * 16 + fq + 4 * r] = big[r];
        if ((lane & 3) == 0) p[(1 * 32 + s) * 16 + 4 * ((lane >> 2) & 3) + fq] = small;     // D of 4x4x4: j = 0, row 4 b + i
        if (fq == 0) p[(2 * 32 + s) * 16 + fr] = chain;
    }
}

// 3. reps x 32 dependent MFMAs of one form, lane 0 writes the cycles
template <int FORM>
__global__ __launch_bounds__(64) void k_time(double* sink, long long* cyc, int reps)
{
    const int lane = threadIdx.x;
    const double a = 1.0 + lane * 1e-9, b = 1.0000001;
    Acc big = {0.0, 0.0, 0.0, 0.0};
    double small = 0.0;
    const long long t0 = clock64();
    for (int i = 0; i < reps; ++i) {
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            if constexpr (FORM == 0) big = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, big, 0, 0, 0);
            else small = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, small, 0, 0, 0);
        }
    }
    const long long t1 = clock64();
    if (lane == 0) *cyc = t1 - t0;
    sink[lane] = big[0] + big[1] + big[2] + big[3] + small;
}

static double rnd(uint64_t& s)     // xorshift, uniform in [-1, 1)
{
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    return (double)(int64_t)(s >> 11) / 4503599627370496.0 - 1.0;
}

int main()
{
    // ---- 1. layout
    unsigned long long* dl;
    CK(hipMalloc(&dl, 4096 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_layout, dim3(1), dim3(64), 0, 0, dl);
    CK(hipDeviceSynchronize());
    std::vector<unsigned long long> hl(4096);
    CK(hipMemcpy(hl.data(), dl, 4096 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    int layout_bad = 0;
    for (int la = 0; la < 64; ++la)
        for (int lb = 0; lb < 64; ++lb) {
            const int i = la & 3, ba = (la >> 2) & 3, ka = la >> 4, j = lb & 3, bb = (lb >> 2) & 3, kb = lb >> 4;
            const unsigned long long want = (ba == bb && ka == kb) ? 1ull << (j + 4 * ba + 16 * i) : 0ull;
            if (hl[la * 64 + lb] != want) {
                if (layout_bad < 16) printf("  layout: A lane %d, B lane %d -> D lanes %016llx, assumed %016llx\n", la, lb, hl[la * 64 + lb], want);
                ++layout_bad;
            }
        }
    printf("1. layout of v_mfma_f64_4x4x4_4b_f64 as assumed (A: i + 4 b + 16 k, B: j + 4 b + 16 k, D: j + 4 b + 16 i): %s (%d of 4096 pairs differ)\n",
           layout_bad ? "NO" : "yes", layout_bad);
    if (layout_bad) {                                           // the raw map, for a reader to derive the layout from
        for (int la = 0; la < 64; ++la) {
            printf("  A lane %2d:", la);
            for (int lb = 0; lb < 64; ++lb) if (hl[la * 64 + lb]) printf(" B%d->D%d", lb, __builtin_ctzll(hl[la * 64 + lb]));
            printf("\n");
        }
    }

    // ---- 2. bits
    const int tiles = 4096;
    std::vector<double> hA((size_t)tiles * 16 * 128), hX((size_t)tiles * 128);
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    for (int t = 0; t < tiles; ++t) {
        // a quarter of the tiles each: plain, wide exponent range, cancelling pairs (A columns 2 c and 2 c + 1 nearly opposite), tiny x
        const int kind = t & 3;
        for (int c = 0; c < 128; ++c) hX[(size_t)t * 128 + c] = rnd(seed) * (kind == 3 ? 1e-160 : 1.0);
        for (int r = 0; r < 16; ++r)
            for (int c = 0; c < 128; ++c) {
                double v = rnd(seed);
                if (kind == 1) v = ldexp(v, (int)(rnd(seed) * 40.0));
                hA[((size_t)t * 16 + r) * 128 + c] = v;
            }
        if (kind == 2)
            for (int r = 0; r < 16; ++r)
                for (int c = 0; c < 128; c += 2) {
                    const double x0 = hX[(size_t)t * 128 + c], x1 = hX[(size_t)t * 128 + c + 1];
                    if (x1 != 0.0) hA[((size_t)t * 16 + r) * 128 + c + 1] = -hA[((size_t)t * 16 + r) * 128 + c] * x0 / x1 * (1.0 + 1e-13 * rnd(seed));
                }
    }
    double *dA, *dX, *dP;
    const size_t pn = (size_t)tiles * 3 * 32 * 16;
    CK(hipMalloc(&dA, hA.size() * 8)); CK(hipMalloc(&dX, hX.size() * 8)); CK(hipMalloc(&dP, pn * 8));
    CK(hipMemcpy(dA, hA.data(), hA.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dX, hX.data(), hX.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemset(dP, 0xFF, pn * 8));
    hipLaunchKernelGGL(k_bits, dim3(tiles), dim3(64), 0, 0, dA, dX, dP);
    CK(hipDeviceSynchronize());
    std::vector<double> hP(pn);
    CK(hipMemcpy(hP.data(), dP, pn * 8, hipMemcpyDeviceToHost));
    const char* names[3] = {"16x16x4", "4x4x4_4b", "fma chain (k = 0, 1, 2, 3)"};
    for (int form = 1; form < 3; ++form) {
        long long diff = 0, maxulp = 0;
        int shown = 0;
        for (int t = 0; t < tiles; ++t)
            for (int s = 0; s < 32; ++s)
                for (int r = 0; r < 16; ++r) {
                    int64_t u0, u1;
                    memcpy(&u0, &hP[(((size_t)t * 3 + 0) * 32 + s) * 16 + r], 8);
                    memcpy(&u1, &hP[(((size_t)t * 3 + form) * 32 + s) * 16 + r], 8);
                    if (u0 != u1) {
                        ++diff;
                        const long long d = llabs((long long)(u0 - u1));
                        if (d > maxulp) maxulp = d;
                        if (shown < 4) { printf("  tile %d (kind %d) P_%d row %d: %.17g vs %.17g\n", t, t & 3, s + 1, r, hP[(((size_t)t * 3 + 0) * 32 + s) * 16 + r], hP[(((size_t)t * 3 + form) * 32 + s) * 16 + r]); ++shown; }
                    }
                }
        printf("2. prefixes of %s against %s: %lld of %lld differ (largest distance %lld in the bit pattern)\n", names[form], names[0],
               diff, (long long)tiles * 32 * 16, maxulp);
    }

    // ---- 3. time
    double* sink; long long* cyc;
    CK(hipMalloc(&sink, 64 * 8)); CK(hipMalloc(&cyc, 8));
    const int reps = 2000;
    for (int form = 0; form < 2; ++form) {
        long long h = 0;
        for (int rep = 0; rep < 2; ++rep) {
            if (form == 0) hipLaunchKernelGGL(k_time<0>, dim3(1), dim3(64), 0, 0, sink, cyc, reps);
            else hipLaunchKernelGGL(k_time<1>, dim3(1), dim3(64), 0, 0, sink, cyc, reps);
            CK(hipDeviceSynchronize());
        }
        CK(hipMemcpy(&h, cyc, 8, hipMemcpyDeviceToHost));
        printf("3. one dependent chain of %s: %.1f cycles per MFMA\n", names[form], (double)h / reps / 32);
    }
    return layout_bad ? 1 : 0;
}
