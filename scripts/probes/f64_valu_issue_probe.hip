// f64_valu_issue_probe.hip -- issue cost of the vector instructions of the forked GEMM's epilogue (dtanh, the pair difference,
// the store addresses) that scripts/probes/f64_coexec_probe.hip never covered. One wave alone on its SIMD issues 64 independent
// copies of one instruction per round (16 destinations, the same sources), `reps` rounds, stamped with s_memtime: cycles per
// instruction. A second table runs the same stream in both waves of a SIMD (512 threads, waves w and w + 4 share one).
// Build + run on the GPU box:  hipcc --offload-arch=gfx950 -O3 -o /tmp/f64_valu_issue scripts/probes/f64_valu_issue_probe.hip && /tmp/f64_valu_issue
#include <hip/hip_runtime.h>
#include <cstdio>

#define REP16(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15)

template <int OP>
__device__ __forceinline__ void round16(double (&d)[16], int (&di)[16], double s, int si)
{
#define ONE(i)                                                                                                              \
    if constexpr (OP == 0) asm volatile("v_fma_f64 %0, %1, %1, %1" : "=v"(d[i]) : "v"(s));                                   \
    else if constexpr (OP == 1) asm volatile("v_add_f64 %0, %1, %1" : "=v"(d[i]) : "v"(s));                                  \
    else if constexpr (OP == 2) asm volatile("v_min_f64 %0, %1, %1" : "=v"(d[i]) : "v"(s));                                  \
    else if constexpr (OP == 3) asm volatile("v_rndne_f64 %0, %1" : "=v"(d[i]) : "v"(s));                                    \
    else if constexpr (OP == 4) asm volatile("v_ldexp_f64 %0, %1, %2" : "=v"(d[i]) : "v"(s), "v"(si));                       \
    else if constexpr (OP == 5) asm volatile("v_cvt_i32_f64 %0, %1" : "=v"(di[i]) : "v"(s));                                 \
    else if constexpr (OP == 6) asm volatile("v_rcp_f64 %0, %1" : "=v"(d[i]) : "v"(s));                                      \
    else if constexpr (OP == 7) asm volatile("v_lshl_add_u64 %0, %1, 3, %1" : "=v"(d[i]) : "v"(s));                          \
    else if constexpr (OP == 8) asm volatile("v_lshl_add_u32 %0, %1, 20, %1" : "=v"(di[i]) : "v"(si));                       \
    else if constexpr (OP == 9) asm volatile("v_mov_b32_dpp %0, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=v"(di[i]) : "v"(si)); \
    else if constexpr (OP == 10) asm volatile("v_bfi_b32 %0, %1, %1, %1" : "=v"(di[i]) : "v"(si));                           \
    else if constexpr (OP == 11) asm volatile("v_mul_f64 %0, %1, %1" : "=v"(d[i]) : "v"(s));                                 \
    else asm volatile("v_add_u32 %0, %1, %1" : "=v"(di[i]) : "v"(si));
    REP16(ONE)
#undef ONE
}

constexpr int NOPS = 13;
static const char* op_names[NOPS] = {"v_fma_f64", "v_add_f64", "v_min_f64", "v_rndne_f64", "v_ldexp_f64", "v_cvt_i32_f64", "v_rcp_f64",
                                      "v_lshl_add_u64", "v_lshl_add_u32", "v_mov_b32_dpp", "v_bfi_b32", "v_mul_f64", "v_add_u32"};

// active[w] != 0: wave w runs the stream
template <int OP>
__global__ __launch_bounds__(512) void k(const int* active, double* sink, long long* cyc, int reps)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool on = active[wave] != 0;
    double d[16];
    int di[16];
    for (int i = 0; i < 16; ++i) { d[i] = 0.0; di[i] = 0; }
    const double s = 1.25 + lane * 1e-3;
    const int si = 3 + (lane & 7);
    __syncthreads();
    const long long t0 = clock64();
    if (on)
        for (int r = 0; r < reps; ++r) {
            round16<OP>(d, di, s, si); round16<OP>(d, di, s, si); round16<OP>(d, di, s, si); round16<OP>(d, di, s, si);
        }
    const long long t1 = clock64();
    __syncthreads();
    if (lane == 0) cyc[wave] = on ? t1 - t0 : 0;
    double acc = 0.0;
    for (int i = 0; i < 16; ++i) acc += d[i] + di[i];
    sink[threadIdx.x] = acc;
}

template <int OP>
void run(const int* roles, double* sink, long long* cyc, int reps, double (&res)[NOPS][2])
{
    const int one[8] = {1, 0, 0, 0, 0, 0, 0, 0}, two[8] = {1, 0, 0, 0, 1, 0, 0, 0};
    for (int c = 0; c < 2; ++c) {
        (void)hipMemcpy((void*)roles, c ? two : one, sizeof(one), hipMemcpyHostToDevice);
        for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(k<OP>, dim3(1), dim3(512), 0, 0, roles, sink, cyc, reps);
        (void)hipDeviceSynchronize();
        long long h[8];
        (void)hipMemcpy(h, cyc, sizeof(h), hipMemcpyDeviceToHost);
        const long long worst = h[0] > h[4] ? h[0] : h[4];
        res[OP][c] = (double)worst / reps / 64;
    }
    if constexpr (OP + 1 < NOPS) run<OP + 1>(roles, sink, cyc, reps, res);
}

int main()
{
    int* roles; double* sink; long long* cyc;
    if (hipMalloc(&roles, 8 * sizeof(int)) != hipSuccess) { printf("no device\n"); return 2; }
    (void)hipMalloc(&sink, 512 * sizeof(double)); (void)hipMalloc(&cyc, 8 * sizeof(long long));
    const int reps = 2000;
    double res[NOPS][2];
    run<0>(roles, sink, cyc, reps, res);
    printf("cycles per instruction, 64 independent per round, %d rounds\n%-18s %12s %28s\n", reps, "instruction", "one wave", "both waves of the SIMD, each");
    for (int o = 0; o < NOPS; ++o) printf("%-18s %12.2f %28.2f\n", op_names[o], res[o][0], res[o][1]);
    return 0;
}
