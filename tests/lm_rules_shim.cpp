// extern "C" doors to csrc/lm_rules.h for tests/test_lm_rules.py: plain host C++, float (_s) and double (_d)
#include "mir_optim_amd.h"
#include "../mir_optim_amd/csrc/lm_rules.h"

using namespace mirlsq;

extern "C" int lmr_suspicious_mu() { return kSuspiciousMu; }
#define SHIM(T, S, SET)                                                                                                        \
    extern "C" void lmr_reject_##S(T* lambda, T* mu, const SET* s) { LM_REJECT(*lambda, *mu, lm_settings_dev(s)); }            \
    extern "C" void lmr_rate_step_##S(T rho, T* lambda, T* mu, const SET* s) { LM_RATE_STEP(rho, *lambda, *mu, lm_settings_dev(s)); } \
    extern "C" T lmr_lambda0_##S(T d_first, const SET* s) { T l; LM_LAMBDA0(l, d_first, lm_settings_dev(s)); return l; }      \
    extern "C" void lmr_settings_dev_##S(const SET* s, T* out14, uint32_t* out2)                                               \
    {                                                                                                                          \
        const LmSettingsDev<T> d = lm_settings_dev(s);                                                                         \
        const T f[14] = {d.jacobianEpsilon, d.absTolerance, d.relTolerance, d.gradTolerance, d.maxGoodResidual, d.maxStep, d.maxLambda, \
                         d.minLambda, d.minStepQuality, d.goodStepQuality, d.lambdaIncrease, d.lambdaDecrease, d.qpRelTolerance, \
                         d.qpAbsTolerance};                                                                                    \
        for (int i = 0; i < 14; ++i) out14[i] = f[i];                                                                          \
        out2[0] = d.qpMaxIterations; out2[1] = d.pad;                                                                          \
    }
SHIM(double, d, mir_least_squares_settings_d)
SHIM(float, s, mir_least_squares_settings_s)
