// workloads_gemm.h -- which kernel a tanh-linear call runs (tl_class: ONE statement of the choice, which the C entries in
// workloads.hip switch on and wl_tanh_linear_class exports), and the launchers of the batched residual GEMM (workloads_gemm.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

// the entries: f (one point), g (its analytic Jacobian), fb (p points, point-major), fbr (row-major), fbd (difference panel)
enum : int { TL_OP_F = 0, TL_OP_G = 1, TL_OP_FB = 2, TL_OP_FBR = 3, TL_OP_FBD = 4 };
// the kernel families: k_tanh_linear, k_tanh_linear_rows, k_tanh_linear_multi, k_tanh_linear_batched, k_tanh_linear_batched_dma,
// k_tanh_linear_batched_wide, k_tanh_linear_batched_rm_generic, k_tanh_linear_batched_diff_generic; LOOP: fb's one-point sweep
// per point (width and flags are that sweep's: k_tanh_linear, or k_tanh_linear_rows with width 0)
enum : int { TL_SWEEP = 0, TL_ROWS = 1, TL_MULTI = 2, TL_MFMA = 3, TL_DMA = 4, TL_WIDE = 5, TL_GENERIC_RM = 6, TL_GENERIC_DIFF = 7, TL_LOOP = 8 };
// flags: VEC (SWEEP: 16-byte loads of A; DMA point-major: 16-byte stores of Y), RM / DIFF / BASE (the DMA kernel's template
// arguments), and from bit 4 the mode: MODE of SWEEP / ROWS (1: Jacobian); for a DMA difference panel the mode that takes effect
// (0 chunked sweep, 1 A read once, 2 prefix forking -- when X passes the kernel's structure vote, else the chunked sweep)
enum : int { TL_VEC = 1, TL_RM = 2, TL_DIFF = 4, TL_BASE = 8, TL_MODE_SHIFT = 4 };

struct TlClass {
    int family;
    int width;       // SWEEP, MULTI: NCP; MFMA, DMA: NK; WIDE: OUT; else 0
    int flags;
    int launches;    // kernel launches of the call (LOOP: p; a p = 2n + 1 difference panel whose extra point is not folded: 2)
};

inline TlClass tl_class_point(size_t n, unsigned aA, int elem, int mode)
{
    const int ncp = (int)((n + 31) / 32);
    if (ncp > 8) return {TL_ROWS, 0, mode << TL_MODE_SHIFT, 1};
    const bool vec = n % 2 == 0 && aA % (2 * elem) == 0;
    return {TL_SWEEP, ncp <= 1 ? 1 : ncp <= 2 ? 2 : ncp <= 4 ? 4 : 8, (vec ? TL_VEC : 0) | (mode << TL_MODE_SHIFT), 1};
}

// aA, aX, aY: the addresses of A, X (x) and Y (y, J, D) modulo 16; elem: 8 (double) or 4 (float: f and g only).
// dma = false: the choice when the DMA kernel's LDS size cannot be set (hipFuncSetAttribute failed: launch_tlb_dma_class)
inline TlClass tl_class(int op, size_t m, size_t n, size_t p, unsigned aA, unsigned aX, unsigned aY, int elem, int read_a_once,
                        int dense, bool dma = true)
{
    if (op == TL_OP_F || op == TL_OP_G) return tl_class_point(n, aA, elem, op == TL_OP_G);
    const int nk = n == 256 ? 64 : n == 128 ? 32 : n == 64 ? 16 : n == 32 ? 8 : 0;      // the DMA kernel's shapes
    const bool wide = n > 256 && n % 8 == 0 && m > 0;
    if (op == TL_OP_FB) {
        if (p <= 8 && n <= 128 && n % 2 == 0 && aA == 0 && aX == 0) return {TL_MULTI, n <= 32 ? 1 : n <= 64 ? 2 : 4, 0, 1};
        const int vec = (m % 2 == 0 && aY == 0) ? TL_VEC : 0;
        if (n == 256 && m >= 32 && dma) return {TL_DMA, 64, vec, 1};
        if (wide) return {TL_WIDE, 2, 0, 1};
        if (n % 2 != 0 || n > 128 || n < 4) {
            const TlClass c = tl_class_point(n, aA, 8, 0);
            return {TL_LOOP, c.width, c.flags, (int)p};
        }
        if (m >= 32 && nk && dma) return {TL_DMA, nk, vec, 1};
        return {TL_MFMA, n <= 16 ? 4 : n <= 32 ? 8 : n <= 64 ? 16 : 32, 0, 1};
    }
    if (op == TL_OP_FBR) {
        if (m >= 32 && nk && dma) return {TL_DMA, nk, TL_RM, 1};
        if (wide) return {TL_WIDE, 0, 0, 1};
        return {TL_GENERIC_RM, 0, 0, 1};
    }
    // the difference panel; p = 2n + 1: one more point behind the 2n, folded into the n = 128 kernel or swept on its own
    const bool base = p == 2 * n + 1;
    const size_t P = base ? 2 * n : p;
    const int extra = base ? 1 : 0;
    if (m >= 32 && P % 16 == 0 && nk && dma) {
        const int mode = read_a_once ? 1 : dense ? 0 : 2;
        const int eff = (mode == 1 && nk <= 32 && P == 2 * n) ? 1 : (mode == 2 && nk == 32 && P == 2 * n) ? 2 : 0;
        if (base && n == 128 && mode != 1) return {TL_DMA, 32, TL_RM | TL_DIFF | TL_BASE | (eff << TL_MODE_SHIFT), 1};
        return {TL_DMA, nk, TL_RM | TL_DIFF | (eff << TL_MODE_SHIFT), 1 + extra};
    }
    if (wide && P % 2 == 0) return {TL_WIDE, 1, 0, 1 + extra};
    return {TL_GENERIC_DIFF, 0, 0, 1 + extra};
}

// the DMA kernel of class c (family TL_DMA) on P points; false, and nothing launched, when its LDS size cannot be set.
// read_a_once, dense: what the entry was given (the kernel's mode argument: 1, 0, else 2)
bool launch_tlb_dma_class(const TlClass& c, const double* A, const double* b, const double* X, double* Y, size_t m, int P, hipStream_t s,
                          int read_a_once, bool dense);
// the MFMA, WIDE and GENERIC kernels of class c
void launch_tanh_linear_gemm_class(const TlClass& c, const double* A, const double* b, const double* X, double* Y, size_t m, int n, int P,
                                   hipStream_t s);
