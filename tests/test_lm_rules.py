"""csrc/lm_rules.h -- the one statement of the damping schedule, which every kernel and the host loop expand -- against the
independent CPU oracle (oracle/, which shares no line with it). CPU tier: tests/lm_rules_shim.cpp wraps the rules for the system
C++ compiler; the oracle runs small problems with NON-default settings and a trace, and every damping it used must be what the
rules make of the one before, bit for bit:
  * a rejection (trace events 2: no improvement, 4: step guard) followed by another pass on the same Jacobian: the next
    lambda is LM_REJECT's, mu doubling from its value after the last acceptance (LS:1103-1104, 1127-1128);
  * an acceptance (event 3): the next lambda is one of LM_RATE_STEP's three outcomes (LS:1152-1161; rho is not in the trace);
  * the first lambda of a fit is LM_LAMBDA0 of the first maximal diagonal entry of J^T J at x0 (LS:1067-1072);
  * lm_settings_dev copies all 15 fields.
Each case must hold at least three rejections and one acceptance of good quality, or it fails instead of passing vacuously."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import problems as P
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "lm_rules_shim.cpp")
HDR = os.path.join(ROOT, "mir_optim_amd", "csrc", "lm_rules.h")
LIB = os.path.join(ROOT, "tests", "liblm_rules_shim.so")

NON_DEFAULT = dict(lambdaIncrease=1.5, lambdaDecrease=0.5, minLambda=1e-6, minStepQuality=0.2, goodStepQuality=0.6)


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "include"), SRC, "-o", LIB])
    L = C.CDLL(LIB)
    L.lmr_suspicious_mu.restype = C.c_int
    for suf, ct, st in (("d", C.c_double, O.SettingsD), ("s", C.c_float, O.SettingsS)):
        sp, tp = C.POINTER(st), C.POINTER(ct)
        for name, res, args in (("reject", None, [tp, tp, sp]), ("rate_step", None, [ct, tp, tp, sp]), ("lambda0", ct, [ct, sp]),
                                ("settings_dev", None, [sp, C.c_void_p, C.c_void_p])):
            fn = getattr(L, "lmr_%s_%s" % (name, suf))
            fn.restype, fn.argtypes = res, args
    return L


def _settings(dtype):
    s = O.default_settings(dtype)
    for k, v in NON_DEFAULT.items():
        setattr(s, k, v)
    return s


CASES = [("t3a", np.float64), ("t3a", np.float32), ("t3b", np.float64)]


@pytest.mark.parametrize("name,dtype", CASES, ids=["%s-%s" % (n, np.dtype(d).name) for n, d in CASES])
def test_oracle_trace_follows_the_shared_rules(shim, name, dtype):
    p = getattr(P, name)()
    suf = "d" if dtype == np.float64 else "s"
    S = _settings(dtype)
    ev = []
    O.optimize(p["f"], p["m"], p["x0"], p["lower"], p["upper"], g=p["g"], settings=S, dtype=dtype,
               trace=lambda e, it, lam, res, tres, dxd: ev.append((e, dtype(lam))))
    T, ct = dtype, (C.c_double if dtype == np.float64 else C.c_float)

    def rule(name, lam, mu, *rho):                                 # (lambda, mu) after LM_REJECT / LM_RATE_STEP
        l, m_ = ct(lam), ct(mu)
        getattr(shim, "lmr_%s_%s" % (name, suf))(*rho, C.byref(l), C.byref(m_), S)
        return T(l.value), T(m_.value)
    # lambda_0: J at x0 from the problem's own g, J^T J's diagonal in the oracle's type (two rows: one addition, no order to choose)
    assert p["m"] == 2
    J = np.zeros((2, len(p["x0"])), dtype=dtype)
    p["g"](np.array(p["x0"], dtype=dtype), J)
    diag = (J * J)[0] + (J * J)[1]
    first = [lam for e, lam in ev if e in (2, 3, 4)][0]
    assert ev[0] == (0, T(0))
    assert first == T(getattr(shim, "lmr_lambda0_" + suf)(diag[np.argmax(np.abs(diag))], S))
    mid = (S.minStepQuality + S.goodStepQuality) / 2
    mu, rejections, good, poor, checked = T(1), 0, 0, 0, 0
    for (e, lam), (e2, lam2) in zip(ev, ev[1:]):
        if e in (2, 4):                                            # a rejection
            rejections += 1
            want, mu = rule("reject", lam, mu)
            if e2 in (2, 3, 4):                                    # the next pass solves on the same Jacobian
                assert lam2 == want, (e, lam, mu, lam2, want)
                checked += 1
            elif mu > shim.lmr_suspicious_mu():                    # LS:984: the forced refresh (event 0) resets mu
                assert e2 == 0
                mu = T(1)
        elif e == 3:                                               # an acceptance (mu = 1): the next event shows the rated lambda
            out = {rho: rule("rate_step", lam, 1, ct(rho)) for rho in (0.0, mid, 1.0)}
            assert out[mid] == (lam, 1) and out[0.0][1] == 2 and out[1.0][1] == 1
            took = [rho for rho in (0.0, mid, 1.0) if out[rho][0] == lam2]
            assert took, (lam, lam2, out)
            good += took == [1.0]
            poor += took == [0.0]
            mu = out[took[0]][1]
    print("rejections %d, checked %d, good-quality acceptances %d, poor-quality %d" % (rejections, checked, good, poor))
    assert rejections >= 3 and checked >= 2 and good >= 1, (rejections, checked, good)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_settings_copy_takes_all_fifteen_fields(shim, dtype):
    S = O.SettingsD() if dtype == np.float64 else O.SettingsS()
    S.maxIterations, S.maxAge = 901, 902                           # not part of the device copy
    for i, k in enumerate(O._FIELDS):
        setattr(S, k, 1.5 + i)
    S.qpSettings.relTolerance, S.qpSettings.absTolerance, S.qpSettings.maxIterations = 13.5, 14.5, 77
    out, u = np.full(14, -1, dtype=dtype), np.full(2, 9, dtype=np.uint32)
    getattr(shim, "lmr_settings_dev_" + ("d" if dtype == np.float64 else "s"))(C.byref(S), out.ctypes.data, u.ctypes.data)
    assert out.tolist() == [1.5 + i for i in range(14)]
    assert u.tolist() == [77, 0]
