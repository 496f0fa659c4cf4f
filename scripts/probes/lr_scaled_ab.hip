// lr_scaled_ab.hip -- what does it cost to keep J0 as the unscaled difference panel? HIP events on the kernels alone, cases
// interleaved, ROUNDS rounds of REPS launches each, ms per launch (median, min .. max over the rounds):
//   the fused FD kernel of the difference panel (jtj_run) with Jout = J (JtjOp::fd_diff) and with Jout = nullptr (fd_diff_keep);
//   the read-only Broyden sweep (lr_sweep) over J and over the panel with twh (the scaled instance), at k = 1 and k = 4.
// The break-even of a solve with 2 refreshes and 4 sweeps: the FD kernel's saving must exceed twice the sweep's loss.
// Build (from the repository root, after the library) + run on the GPU box:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o scripts/probes/lr_scaled_ab scripts/probes/lr_scaled_ab.hip \
//         -Lmir_optim_amd/lib -lmir_optim_amd -Wl,-rpath,'$ORIGIN/../../mir_optim_amd/lib'
//   scripts/probes/lr_scaled_ab [m = 1000000] [n = 128]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mir_optim_amd/csrc/broyden_launch.h"
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
    if (m == 0 || n < 2 || n > kLrScaledMaxN || n % 2) { std::fprintf(stderr, "m > 0, n even, 2 <= n <= %d\n", kLrScaledMaxN); return 1; }
    int dev = 0, num_cu = 0;
    CHECK(hipGetDevice(&dev));
    CHECK(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev));
    const JtjPlan plan = jtj_plan<double>(m, n, num_cu);
    if (plan.of(JtjOp::fd_diff).kernel == JtjKernel::none) { std::fprintf(stderr, "no difference-panel kernel for n = %d\n", n); return 1; }
    const int nblk = lr_blocks(m, num_cu), len = lr_len(n);
    double *P, *J, *twh, *y, *yold, *U, *D, *dx, *dxdot, *part, *slabs, *packed;
    CHECK(hipMalloc((void**)&P, m * n * sizeof(double)));
    CHECK(hipMalloc((void**)&J, m * n * sizeof(double)));
    CHECK(hipMalloc((void**)&twh, n * sizeof(double)));
    CHECK(hipMalloc((void**)&y, m * sizeof(double)));
    CHECK(hipMalloc((void**)&yold, m * sizeof(double)));
    CHECK(hipMalloc((void**)&U, (size_t)kLrMax * m * sizeof(double)));
    CHECK(hipMalloc((void**)&D, (size_t)kLrMax * n * sizeof(double)));
    CHECK(hipMalloc((void**)&dx, n * sizeof(double)));
    CHECK(hipMalloc((void**)&dxdot, sizeof(double)));
    CHECK(hipMalloc((void**)&part, (size_t)nblk * len * sizeof(double)));
    CHECK(hipMalloc((void**)&slabs, jtj_slab_elems(plan) * sizeof(double)));
    CHECK(hipMalloc((void**)&packed, ((size_t)n * (n + 1) / 2 + n + 8) * sizeof(double)));
    hipLaunchKernelGGL(k_fill, dim3(1024), dim3(256), 0, nullptr, P, m * n, 1u, 1e-6);
    hipLaunchKernelGGL(k_fill, dim3(256), dim3(256), 0, nullptr, y, m, 2u, 1.0);
    hipLaunchKernelGGL(k_fill, dim3(256), dim3(256), 0, nullptr, yold, m, 3u, 1.0);
    hipLaunchKernelGGL(k_fill, dim3(256), dim3(256), 0, nullptr, U, (size_t)kLrMax * m, 4u, 1.0);
    hipLaunchKernelGGL(k_fill, dim3(16), dim3(256), 0, nullptr, D, (size_t)kLrMax * n, 5u, 1e-3);
    hipLaunchKernelGGL(k_fill, dim3(1), dim3(256), 0, nullptr, dx, (size_t)n, 6u, 1e-3);
    std::vector<double> th(n, 2e-6);
    th[n / 2] = 0.0;                                       // one collapsed interval
    const double dd = 1e-4;
    CHECK(hipMemcpy(twh, th.data(), n * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dxdot, &dd, sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipDeviceSynchronize());

    JtjArgs<double> ja{};
    ja.J = P; ja.Jout = J; ja.y = y; ja.y_old = y; ja.slabs = slabs; ja.m = m; ja.n = n; ja.twh = twh;
    LrArgs<double> la{};
    la.U = U; la.D = D; la.dx = dx; la.dx_dot = dxdot; la.y = y; la.y_old = yold; la.partials = part; la.m = m; la.n = n;

    enum { FD_WRITE, FD_NOWRITE, LR_PLAIN_1, LR_SCALED_1, LR_PLAIN_4, LR_SCALED_4, NCASE };
    const char* names[NCASE] = {"k_jtj_fdp, Jout = J", "k_jtj_fdp, Jout = nullptr", "sweep over J, k = 1", "sweep over the panel, k = 1",
                                "sweep over J, k = 4", "sweep over the panel, k = 4"};
    auto run = [&](int c) -> hipError_t {
        if (c == FD_WRITE || c == FD_NOWRITE) {
            JtjArgs<double> a = ja;
            if (c == FD_NOWRITE) a.Jout = nullptr;
            return jtj_run<double>(plan, c == FD_NOWRITE ? JtjOp::fd_diff_keep : JtjOp::fd_diff, a, packed, nullptr);
        }
        LrArgs<double> a = la;
        a.k = (c == LR_PLAIN_1 || c == LR_SCALED_1) ? 1 : 4;
        const bool scaled = c == LR_SCALED_1 || c == LR_SCALED_4;
        a.J = scaled ? P : J;
        return lr_sweep<double>(a, nblk, nullptr, scaled ? twh : nullptr);
    };
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int c = 0; c < NCASE; ++c) CHECK(run(c));         // warm-up; FD_WRITE fills J with the scaled panel
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
    double med[NCASE];
    for (int c = 0; c < NCASE; ++c) {
        std::sort(ms[c].begin(), ms[c].end());
        med[c] = ms[c][ROUNDS / 2];
        std::printf("  %-30s %.4f (%.4f .. %.4f)\n", names[c], med[c], ms[c].front(), ms[c].back());
    }
    const double save = med[FD_WRITE] - med[FD_NOWRITE];
    const double loss1 = med[LR_SCALED_1] - med[LR_PLAIN_1], loss4 = med[LR_SCALED_4] - med[LR_PLAIN_4];
    std::printf("FD kernel saves %.4f ms per launch; the scaled sweep costs %.4f (k = 1), %.4f (k = 4) ms per launch\n", save, loss1, loss4);
    std::printf("per solve (2 refreshes, 4 sweeps): %.4f ms saved, %.4f ms lost -> %s\n", 2 * save, 4 * std::max(loss1, loss4),
                save > 2 * std::max(loss1, loss4) ? "worth it" : "NOT worth it");
    return 0;
}
