// jtj_store_free_ab.hip -- the fused FD kernel alone, for an A/B of two trees (profiles/r26): HIP events, ROUNDS rounds of REPS
// launches each, cases interleaved, ms per launch (median, min .. max over the rounds), the method of lr_scaled_ab.hip:
//   the difference panel with Jout = nullptr (JtjOp::fd_diff_keep: k_jtj_fdp_nw at n % 16 == 0, n <= 128; k_jtj_fdp8 above) and with Jout = J,
//   and the plain J^T J of the J that the second case wrote.
// Every figure includes the slab reduction that jtj_run launches behind the kernel (a few microseconds, the same in both trees).
// Build it in EACH tree against that tree's library (from the tree's root, after the library) and run the two alternately:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o scripts/probes/jtj_store_free_ab scripts/probes/jtj_store_free_ab.hip \
//         -Lmir_optim_amd/lib -lmir_optim_amd -Wl,-rpath,'$ORIGIN/../../mir_optim_amd/lib'
//   scripts/probes/jtj_store_free_ab [m = 1000000] [n = 128]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mir_optim_amd/csrc/jtj_plan.h"

using namespace mirlsq;

#define CHECK(e) do { hipError_t err_ = (e); if (err_ != hipSuccess) { std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorName(err_)); return 1; } } while (0)

__global__ void k_fill(double* p, size_t count, unsigned seed, double scale)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)(i * 2654435761u) ^ seed;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        p[i] = scale * ((double)(h & 0xffffff) / 8388608.0 - 1.0);
    }
}

int main(int argc, char** argv)
{
    const size_t m = argc > 1 ? (size_t)std::atoll(argv[1]) : 1000000;
    const int n = argc > 2 ? std::atoi(argv[2]) : 128;
    constexpr int ROUNDS = 5, REPS = 20;
    if (m == 0 || n < 2 || n % 2) { std::fprintf(stderr, "m > 0, n even\n"); return 1; }
    int dev = 0, num_cu = 0;
    CHECK(hipGetDevice(&dev));
    CHECK(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev));
    const JtjPlan plan = jtj_plan<double>(m, n, num_cu);
    if (plan.of(JtjOp::fd_diff).kernel == JtjKernel::none) { std::fprintf(stderr, "no difference-panel kernel for n = %d\n", n); return 1; }
    double *P, *J, *twh, *y, *slabs, *packed;
    CHECK(hipMalloc((void**)&P, m * n * sizeof(double)));
    CHECK(hipMalloc((void**)&J, m * n * sizeof(double)));
    CHECK(hipMalloc((void**)&twh, n * sizeof(double)));
    CHECK(hipMalloc((void**)&y, m * sizeof(double)));
    CHECK(hipMalloc((void**)&slabs, jtj_slab_elems(plan) * sizeof(double)));
    CHECK(hipMalloc((void**)&packed, ((size_t)n * (n + 1) / 2 + n + 8) * sizeof(double)));
    hipLaunchKernelGGL(k_fill, dim3(1024), dim3(256), 0, nullptr, P, m * n, 1u, 1e-6);
    hipLaunchKernelGGL(k_fill, dim3(256), dim3(256), 0, nullptr, y, m, 2u, 1.0);
    std::vector<double> th(n, 2e-6);                       // no collapsed interval, as in the benchmark's solves
    CHECK(hipMemcpy(twh, th.data(), n * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipDeviceSynchronize());

    JtjArgs<double> fa{};
    fa.J = P; fa.Jout = J; fa.y = y; fa.y_old = y; fa.slabs = slabs; fa.m = m; fa.n = n; fa.twh = twh;
    JtjArgs<double> pa = fa;
    pa.J = J; pa.Jout = J; pa.twh = nullptr;

    enum { FD_NULL, FD_WRITE, PLAIN, NCASE };
    const char* names[NCASE] = {"difference panel, Jout = nullptr", "difference panel, Jout = J", "plain J^T J"};
    auto run = [&](int c) -> hipError_t {
        if (c == PLAIN) return jtj_run<double>(plan, JtjOp::plain, pa, packed, nullptr);
        JtjArgs<double> a = fa;
        if (c == FD_NULL) a.Jout = nullptr;
        return jtj_run<double>(plan, c == FD_NULL ? JtjOp::fd_diff_keep : JtjOp::fd_diff, a, packed, nullptr);
    };
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    CHECK(run(FD_WRITE));                                  // fills J for the plain case
    for (int c = 0; c < NCASE; ++c)                        // warm-up: one untimed round (the first round after the allocations runs
        for (int i = 0; i < REPS; ++i) CHECK(run(c));      // 15 to 20 % slow in either tree)
    CHECK(hipDeviceSynchronize());
    std::vector<float> ms[NCASE];
    for (int r = 0; r < ROUNDS; ++r)
        for (int c = 0; c < NCASE; ++c) {
            CHECK(hipEventRecord(e0, nullptr));
            for (int i = 0; i < REPS; ++i) CHECK(run(c));
            CHECK(hipEventRecord(e1, nullptr));
            CHECK(hipEventSynchronize(e1));
            float t = 0;
            CHECK(hipEventElapsedTime(&t, e0, e1));
            ms[c].push_back(t / REPS);
        }
    std::printf("m = %zu, n = %d, %d CUs, %d rounds of %d launches, ms per launch: median (min .. max)\n", m, n, num_cu, ROUNDS, REPS);
    for (int c = 0; c < NCASE; ++c) {
        std::sort(ms[c].begin(), ms[c].end());
        std::printf("  %-34s %.4f (%.4f .. %.4f)\n", names[c], ms[c][ROUNDS / 2], ms[c].front(), ms[c].back());
    }
    return 0;
}
