// lm_rules.h -- the ONE statement of the Levenberg-Marquardt damping schedule and exit tests of optimizeLeastSquaresImplGeneric!T
// (least_squares.d, cited as LS:line). The host round loop (solver_loop.hip), the decision kernel (misc_kernels.h), the resident-J
// loop (resident_kernel.h), the wave-per-problem kernel (batched_kernel.h), the solves (solve_kernel.h, solve_big.h,
// solve_wave16.h) and the ladder builders that precompute what a rejection will do all expand these; none spells a rule out.
// They are MACROS on purpose: an inlined function is simplified before it is inlined, and at these sites that turned compares
// round and renamed registers (profiles/r09). A macro is the parent's expression, token for token, so the kernels compile to
// the parent's code. Arguments: lvalues where a rule assigns (lambda, mu), `set` anything with LmSettingsDev's members.
// Plain C++: tests/lm_rules_shim.cpp wraps each rule for the system compiler, tests/test_lm_rules.py holds them to the CPU oracle.
#pragma once

#include <cmath>
#include <cstdint>

namespace mirlsq {

template <typename T>
struct LmSettingsDev {   // the floating-point part of LeastSquaresSettings!T (LS:85-123)
    T jacobianEpsilon, absTolerance, relTolerance, gradTolerance, maxGoodResidual, maxStep, maxLambda,
      minLambda, minStepQuality, goodStepQuality, lambdaIncrease, lambdaDecrease, qpRelTolerance, qpAbsTolerance;
    uint32_t qpMaxIterations, pad;
};

// LeastSquaresSettings!T as the C ABI lays it out (mir_least_squares_settings_d / _s) -> the kernels' copy, all 15 fields
template <class Settings>
inline auto lm_settings_dev(const Settings* S) -> LmSettingsDev<decltype(Settings::jacobianEpsilon)>
{
    LmSettingsDev<decltype(Settings::jacobianEpsilon)> d;
    d.jacobianEpsilon = S->jacobianEpsilon; d.absTolerance = S->absTolerance; d.relTolerance = S->relTolerance;
    d.gradTolerance = S->gradTolerance; d.maxGoodResidual = S->maxGoodResidual; d.maxStep = S->maxStep;
    d.maxLambda = S->maxLambda; d.minLambda = S->minLambda; d.minStepQuality = S->minStepQuality;
    d.goodStepQuality = S->goodStepQuality; d.lambdaIncrease = S->lambdaIncrease; d.lambdaDecrease = S->lambdaDecrease;
    d.qpRelTolerance = S->qpSettings.relTolerance; d.qpAbsTolerance = S->qpSettings.absTolerance;
    d.qpMaxIterations = S->qpSettings.maxIterations; d.pad = 0;
    return d;
}

constexpr int kSuspiciousMu = 16;        // LS:970, 984: mu beyond it (and an aged Jacobian) forces a refresh

// The tests are written the way the reference writes them inside its `if (!(...))`: NaN fails each of them.
#define LM_F_CONVERGED(residual, set) ((residual) <= (set).maxGoodResidual)                          /* LS:1138 -> 974 */
#define LM_LAMBDA_IN_RANGE(lambda, set) ((lambda) <= (set).maxLambda)                                /* LS:979 */
#define LM_LAMBDA_SET(lambda, set) ((lambda) >= (set).minLambda)                                     /* LS:1067, 1070 */
#define LM_STEP_ALLOWED(dxn, set) ((dxn) < (set).maxStep)                                            /* LS:1101, dxn = ||dx||_2 */
/* LS:1164 (quirk Q6): the step still counts beside x; dxn = ||dx||_2, xnorm = ||x||_2, each caller's own norm */
#define LM_X_MOVING(dxn, xnorm, set) ((dxn) > (set).absTolerance && (xnorm) > (dxn) * (set).relTolerance)
/* LS:974, 1175, 979: none of the top-of-pass tests keeps the next pass from starting */
#define LM_PASS_MAY_START(residual, lambda, iterations, maxIterations, set) \
    (!LM_F_CONVERGED(residual, set) && (iterations) < (maxIterations) && LM_LAMBDA_IN_RANGE(lambda, set))
/* LS:1069-1071: lambda_0 from d_first, the FIRST diagonal entry of J^T J of maximum modulus (each caller's own search) */
#define LM_LAMBDA0(lambda, d_first, set) \
    do { lambda = decltype(lambda)(0.001) * (d_first); if (!LM_LAMBDA_SET(lambda, set)) lambda = 1; } while (0)
/* LS:1103-1104 = 1127-1128 = 1154-1155: what a rejection does to (lambda, mu) */
#define LM_REJECT(lambda, mu, set) do { lambda *= (set).lambdaIncrease * mu; mu *= 2; } while (0)
/* LS:1152-1161: what the quality rho = predicted / actual improvement (quirk Q2) of an accepted step does to (lambda, mu) */
#define LM_RATE_STEP(rho, lambda, mu, set)                                                           \
    do {                                                                                             \
        if ((rho) < (set).minStepQuality) LM_REJECT(lambda, mu, set);                                \
        else if ((rho) >= (set).goodStepQuality) lambda = std::fmax((set).lambdaDecrease * lambda * mu, (set).minLambda); \
    } while (0)

}  // namespace mirlsq
