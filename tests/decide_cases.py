"""Cells, reference and named assertions for the decision kernel of the general solver's round (k_decide_chain, csrc/misc_kernels.h)
run ONE launch at a time through M.lmDecide (mir_lsq_decide_d / _s). tests/test_gpu_decide_cells.py runs them on the device,
tests/test_decide_cell_coverage.py keeps on the CPU that they reach every branch and that the assertions catch planted mistakes.

THE REFERENCE is `walk`: least_squares.d:1080-1161 over a ladder of speculative trials, written from the D source -- not from
lm_rules.h or misc_kernels.h -- in numpy scalars of the cell's type, in the source's operation order: `lambda *= lambdaIncrease * mu`
is lambda (inc mu), `lambdaDecrease * lambda * mu` goes left to right. What the D loop does not have -- the counters the host books,
spec_ok, the sums' second stage -- is restated from the documents of those fields (solve_types.h). The walk is scalar
arithmetic without a reduction, the build has no fast-math option and rho's division is correctly rounded, so EVERY state field,
x, dx_acc and sums are compared BIT FOR BIT (`compare`); a bit of difference is a finding, not a tolerance to add.

THE NOTATION: one token a ladder entry.
  A M P   accepted; rho >= goodStepQuality / between / < minStepQuality        N N- Nn  accepted; predicted 0 / negative / NaN
  R       trial > residual      E  trial == residual       I  trial = +inf (a rejection: LS:1117 lets it pass)       F  trial NaN
  G       step guard (its sum goes in as NaN and is never read)       Z  null step: its sum goes in as NaN and comes back as the residual
  Q1 Q2   qp_status 1 / 2       D  kFlagDxNaN       X  garbage behind an acceptance: NaN sum, qp_status 2 (x: kFlagCoopRescued too)
  g       (first or third entry) kFlagGradSmall on an R entry
"""
import collections
import os
import sys

import numpy as np

import mir_optim_amd as M
from mir_optim_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_lm_rules import NON_DEFAULT as _ND  # noqa: E402

DTYPES = (np.float32, np.float64)
# NON_DEFAULT of test_lm_rules.py plus a maxLambda the rejection chains cross (from lambda 1: 1.5, 4.5, 27, 324 > 64); its
# minLambda (1e-6) is crossed by a good acceptance from LAM_SMALL
SETTINGS = {"default": {}, "nondefault": dict(_ND, maxLambda=64.0)}
LAM = {"default": 0.125, "nondefault": 1.0}
LAM_SMALL = 1.5e-6
MU_ODD = 0.7            # not a power of two: lambda (inc mu) and (lambda inc) mu then differ in their last bits (1.3 does not show it)
RESIDUAL = 100.0
FLAG_DX_NAN, FLAG_X_NAN, FLAG_GUARD, FLAG_NOT_FINITE, FLAG_GRAD, FLAG_NULL, FLAG_RESCUED = 1, 2, 4, 8, 16, 32, 64
SETTING_FIELDS = ("absTolerance", "relTolerance", "maxGoodResidual", "maxLambda", "minLambda", "minStepQuality", "goodStepQuality",
                  "lambdaIncrease", "lambdaDecrease")
PSTRIDE = 1024
NPARTS = (1, 31, 32, 33, 34, 1024)
NS = (1, 7, 255, 256, 257, 300, 1000)

SINGLES = ["A", "M", "P", "N", "N-", "Nn", "R", "E", "I", "F", "G", "Z", "Q1", "Q2", "D"]
CHAINS = [[t] for t in SINGLES] + [list("RRRRRRRR"), list("GRGRGRGA"), list("RRRM"), list("ZZZ"), list("ZRA"), list("RZ"), list("ZR"),
                                   ["R", "R", "Q1"], ["G", "D"], ["R", "F"], ["E", "P"], ["Z", "Q1"],
                                   ["R", "R", "A", "X", "x", "X", "x", "X"]] + [["R"] * j for j in range(2, 8)]
Cell = collections.namedtuple("Cell", "chain dtype settings lam mu lambda_from_state check_grad")


def _cells():
    out = []
    for dt in DTYPES:
        for sname in SETTINGS:
            for ch in CHAINS:
                for mu in (1.0, MU_ODD):
                    out.append(Cell(tuple(ch), dt, sname, LAM[sname], mu, False, False))
            for ch in (["A"], ["R", "R", "A"], ["R"], ["Z", "R", "A"]):                     # lambda_0 arrives through the record
                out.append(Cell(tuple(ch), dt, sname, LAM[sname], 1.0, True, False))
            for ch in (["A"], ["M"], ["R", "A"]):                                             # a good acceptance lands on minLambda
                out.append(Cell(tuple(ch), dt, sname, LAM_SMALL if sname == "nondefault" else 1e-300, 1.0, False, False))
            # the gradient flag: on entry 0 with check_grad (the exit), on entry 0 without it and on entry 2 with it (ignored)
            out.append(Cell(("g", "R", "A"), dt, sname, LAM[sname], MU_ODD, True, True))
            out.append(Cell(("g", "R", "A"), dt, sname, LAM[sname], MU_ODD, False, False))
            out.append(Cell(("R", "R", "g", "A"), dt, sname, LAM[sname], 1.0, False, True))
    return out


CELLS = _cells()


def cell_id(c):
    return "%s-%s-%s-lam%g-mu%g%s%s" % ("".join(c.chain), np.dtype(c.dtype).name, c.settings, c.lam, c.mu,
                                        "-fromrec" if c.lambda_from_state else "", "-grad" if c.check_grad else "")


def settings_of(dtype, overrides):
    s = M.LeastSquaresSettings(dtype)
    for k, v in overrides.items():
        setattr(s, k, v)
    return s


def settings_values(S, dtype):
    """the fields the walk reads, as scalars of the cell's type (the structure holds them in that type already)"""
    return {k: dtype(getattr(S, k)) for k in SETTING_FIELDS}


# ---------------------------------------------------------------------------------------------------------------- inputs
def initial_state(dtype, lam, mu, residual=RESIDUAL, iterations=25):
    """a distinct value in every field"""
    st = np.zeros(1, dtype=api.lm_state_dtype(dtype))
    for i, k in enumerate(api.LM_STATE_FLOATS):
        st[k] = 10.5 + i
    for i, (k, _) in enumerate(api.LM_STATE_INTS):
        st[k] = 21 + i
    st["lambda"], st["mu"], st["residual"], st["iterations"] = lam, mu, residual, iterations
    return st


def entry(token, k, dtype, residual=RESIDUAL):
    """(record fields, sum) of one ladder entry"""
    r = dict(lambda_=1000.0 + k, new_dx_dot=2.0 + k / 8.0, predicted=40.0 + k, trial_xnorm=50.0 + k, qp_status=0, qp_iterations=k % 3,
             flags=0, reserved=7000 + k)
    imp = 10.0
    s = residual - imp
    if token == "A":
        r["predicted"] = 8.0
    elif token == "M":
        r["predicted"] = 3.0
    elif token == "P":
        r["predicted"] = 0.5
    elif token in ("N", "N-", "Nn"):
        r["predicted"] = {"N": 0.0, "N-": -3.0, "Nn": np.nan}[token]
    elif token in ("R", "g"):
        s = residual + 20.0
        if token == "g":
            r["flags"] = FLAG_GRAD
    elif token == "E":
        s = residual
    elif token == "I":
        s = np.inf
    elif token == "F":
        s = np.nan
    elif token == "G":
        r["flags"], s = FLAG_GUARD, np.nan
    elif token == "Z":
        r["flags"], s = FLAG_NULL, np.nan
    elif token in ("Q1", "Q2"):
        r["qp_status"] = int(token[1])
    elif token == "D":
        r["flags"] = FLAG_DX_NAN
    elif token in ("X", "x"):
        r["qp_status"], s = 2, np.nan
        r["flags"] = FLAG_RESCUED if token == "x" else 0
    else:
        raise ValueError(token)
    return r, s


def build(chain, dtype, lam, mu, n=7, nparts=0, seed=0):
    """the operands of one launch: state, rec, sums, x, trial, dx_chain, dx_acc, partials -- every row distinct"""
    ks = len(chain)
    rec = np.zeros(ks, dtype=api.lm_solve_record_dtype(dtype))
    sums = np.zeros(ks, dtype=dtype)
    for k, tok in enumerate(chain):
        r, s = entry(tok, k, dtype)
        for key, v in r.items():
            rec[k]["lambda" if key == "lambda_" else key] = v
        sums[k] = s
    i = np.arange(n)
    kk = np.arange(ks)[:, None]
    ops = dict(state=initial_state(dtype, lam, mu), rec=rec, sums=sums, x=(900000.0 + i).astype(dtype), dx_acc=(800000.0 + i).astype(dtype),
               trial=(1000.0 * (kk + 1) + i + 0.5).astype(dtype), dx_chain=(-1000.0 * (kk + 1) - i - 0.25).astype(dtype), partials=None, nparts=nparts)
    if nparts:
        rng = np.random.default_rng(seed)
        parts = np.full((ks, PSTRIDE), np.nan, dtype=dtype)                # the slots from nparts up hold NaN
        for k in range(ks):
            p = rng.integers(-8, 9, nparts).astype(dtype)                  # exact integers: any order gives the exact sum
            if np.isfinite(sums[k]):
                p[nparts // 2] += sums[k] - p.sum()
            else:
                p[nparts // 2] = sums[k]
            parts[k, :nparts] = p
        ops["partials"] = parts
        ops["sums"] = np.full(ks, -777.0, dtype=dtype)                     # overwritten by the second stage
    return ops


def reduce32(p, nparts):
    """the second stage of the trial sums (32 ranges of ceil(nparts / 32) partials summed in sequence from 0, then the 32
    range totals in sequence) -- the order k_lr_sumsq_final uses, which the fused and the unfused round must share"""
    T = p.dtype.type
    per = (nparts + 31) // 32
    part = []
    for r in range(32):
        s = T(0)
        for b in range(r * per, min(r * per + per, nparts)):
            s = s + p[b]
        part.append(s)
    tot = part[0]
    for r in range(1, 32):
        tot = tot + part[r]
    return tot


# ---------------------------------------------------------------------------------------------------------------- the reference
def ref_reject(T, S, lam, mu, plant=None):
    """LS:1103-1104 = 1127-1128 = 1154-1155"""
    if plant == "assoc":
        return (lam * S["lambdaIncrease"]) * mu, mu * T(2)
    return lam * (S["lambdaIncrease"] * mu), mu * T(2)


def ref_rate(T, S, rho, lam, mu, plant=None):
    """LS:1152-1161; returns (lambda, mu, outcome)"""
    if rho < S["minStepQuality"]:
        return ref_reject(T, S, lam, mu, plant) + ("rate_poor",)
    if rho >= S["goodStepQuality"]:
        return np.fmax(S["lambdaDecrease"] * lam * mu, S["minLambda"]), mu, "rate_good"
    return lam, mu, "rate_mid"


PLANTS = {   # planted mistake -> (a cell that shows it, the name of the assertion that must fail)
    "mu_not_reset": (Cell(("R", "R", "R", "M"), np.float32, "nondefault", 1.0, 1.0, False, False), "mu"),
    "assoc": (Cell(("R", "R", "R"), np.float32, "nondefault", 1.0, MU_ODD, False, False), "lambda"),
    "ge_improvement": (Cell(("E",), np.float64, "default", 0.125, 1.0, False, False), "decision"),
    "inf_error": (Cell(("I",), np.float64, "default", 0.125, 1.0, False, False), "decision"),
    "consumed_past": (Cell(("R", "R", "A", "X", "x", "X", "x", "X"), np.float32, "default", 0.125, 1.0, False, False), "consumed"),
    "null_tail_kept": (Cell(("Z", "R", "A"), np.float64, "nondefault", 1.0, 1.0, False, False), "null_tail"),
    "lambda_from_record": (Cell(("R", "R", "A"), np.float64, "default", 0.125, 1.0, False, False), "lambda"),
    "rescued_to_acceptance": (Cell(("R", "R", "A", "X", "x", "X", "x", "X"), np.float64, "nondefault", 1.0, 1.0, False, False), "coop_rescued"),
    "later_status_leaks": (Cell(("R", "R", "A", "X", "x", "X", "x", "X"), np.float64, "default", 0.125, 1.0, False, False), "qp_status"),
}


def walk(dtype, S, ops, check_grad=False, lambda_from_state=False, spec_static=False, maxIterations=1000, seq=1, mirror=True,
         plant=None):
    """LS:1080-1161 for the ladder of `ops`; returns (result in the shape of M.lmDecide's, path record)"""
    T = np.dtype(dtype).type
    S = S if isinstance(S, dict) else settings_values(S, T)
    st = ops["state"].copy()
    rec, n, ks = ops["rec"], ops["x"].size, ops["rec"].size
    sums = ops["sums"].copy()
    if ops["nparts"]:
        for k in range(ks):
            sums[k] = reduce32(ops["partials"][k], ops["nparts"])
    path = []
    f = {k: T(st[k][0]) for k in api.LM_STATE_FLOATS}
    lam, mu, residual, iterations = f["lambda"], f["mu"], f["residual"], int(st["iterations"][0])
    dec, acc = api.LM_DECIDE_REJECT, -1
    consumed = fcalls = rejects = guards = qpact = null_tail = 0
    with np.errstate(all="ignore"):
        for k in range(ks):
            r = rec[k]
            flags = int(r["flags"])
            if k == 0 and check_grad and flags & FLAG_GRAD:                        # LS:1053: the pass ends before its solve
                dec = api.LM_DECIDE_GRAD_SMALL
                path.append("grad_exit")
                break
            consumed += 1
            if k == 0 and (lambda_from_state or plant == "lambda_from_record"):    # LS:1067-1072 ran in the solve
                lam = T(r["lambda"])
            qpact += int(r["qp_iterations"]) > 0
            st["qp_status"], st["qp_iterations"], st["flags"] = r["qp_status"], r["qp_iterations"], flags
            if int(r["qp_status"]) != 0:                                           # LS:1080-1085
                dec = api.LM_DECIDE_NUMERIC_ERROR
                path.append("qp_failed")
                break
            if flags & FLAG_DX_NAN:                                                # LS:1087-1092
                dec = api.LM_DECIDE_NUMERIC_ERROR
                path.append("dx_nan")
                break
            if flags & FLAG_GUARD:                                                 # LS:1101-1106
                lam, mu = ref_reject(T, S, lam, mu, plant)
                guards += 1
                path.append("guard")
                continue
            fcalls += 1                                                            # LS:1112
            null = bool(flags & FLAG_NULL)
            if null:                                                               # f is pure: f(x) is the vector already held
                sums[k] = residual
                path.append("null")
            null_tail = (null_tail | null) if plant == "null_tail_kept" else int(null)
            tr = T(sums[k])                                                        # LS:1115
            f["trial_residual"] = tr
            if not (tr <= T(np.inf)) or (plant == "inf_error" and not (tr < T(np.inf))):   # LS:1117
                dec = api.LM_DECIDE_NUMERIC_ERROR
                st["flags"] = flags | FLAG_NOT_FINITE
                path.append("not_finite")
                break
            improvement = residual - tr                                            # LS:1124
            f["improvement"] = improvement
            if not ((improvement >= 0) if plant == "ge_improvement" else (improvement > 0)):   # LS:1125-1130
                lam, mu = ref_reject(T, S, lam, mu, plant)
                rejects += 1
                path.append("reject")
                continue
            if plant != "mu_not_reset":
                mu = T(1)                                                          # LS:1133
            iterations += 1
            residual = tr
            f["dx_dot"] = f["new_dx_dot"] = T(r["new_dx_dot"])                     # LS:1139
            f["predicted"], f["trial_xnorm"] = T(r["predicted"]), T(r["trial_xnorm"])
            acc = k
            if not (f["predicted"] > 0):                                           # LS:1144-1148
                dec = api.LM_DECIDE_ACCEPT_NO_PREDICTION
                path.append("no_prediction")
                break
            rho = f["predicted"] / improvement                                     # LS:1150
            f["rho"] = rho
            lam, mu, outcome = ref_rate(T, S, rho, lam, mu, plant)
            path.append(outcome)
            dec = api.LM_DECIDE_ACCEPT
            break
        else:
            path.append("ladder_exhausted")
        if plant == "later_status_leaks":
            st["qp_status"], st["qp_iterations"], st["flags"] = rec[-1]["qp_status"], rec[-1]["qp_iterations"], rec[-1]["flags"]
        spec = 0
        if spec_static and dec == api.LM_DECIDE_ACCEPT and acc == 0:
            # the next pass starts (LS:974, 1175, 979), keeps its lambda (LS:1067) and is a Broyden pass (no flag of the record, LS:1164)
            r = rec[0]
            dxn = np.sqrt(T(r["new_dx_dot"]))
            spec = int(not (residual <= S["maxGoodResidual"]) and iterations < maxIterations and bool(lam <= S["maxLambda"])
                       and bool(lam >= S["minLambda"]) and int(r["qp_status"]) == 0
                       and not (int(r["flags"]) & (FLAG_DX_NAN | FLAG_X_NAN | FLAG_GUARD | FLAG_NULL | FLAG_GRAD))
                       and bool(dxn > S["absTolerance"]) and bool(T(r["trial_xnorm"]) > dxn * S["relTolerance"]))
            path.append("spec_go" if spec else "spec_stop")
    f["lambda"], f["mu"], f["residual"] = lam, mu, residual
    for k, v in f.items():
        st[k] = v
    upto = consumed if plant == "rescued_to_acceptance" else ks
    st["coop_rescued"] = sum(bool(int(rec[k]["flags"]) & FLAG_RESCUED) for k in range(upto))
    st["decision"], st["accepted_k"], st["iterations"], st["spec_ok"] = dec, acc, iterations, spec
    st["consumed"], st["fcalls"], st["rejects"], st["guards"], st["qp_active"] = ks if plant == "consumed_past" else consumed, fcalls, rejects, guards, qpact
    st["null_tail"] = null_tail if (dec == api.LM_DECIDE_REJECT or plant == "null_tail_kept") else 0
    x, dx_acc = ops["x"].copy(), ops["dx_acc"].copy()
    host_state = np.frombuffer(b"\xff" * st.dtype.itemsize, dtype=st.dtype).copy()
    host_x = np.frombuffer(b"\xff" * x.nbytes, dtype=x.dtype).copy()
    if acc >= 0:
        x, dx_acc = ops["trial"][acc].copy(), ops["dx_chain"][acc].copy()          # LS:1135
    if mirror:
        host_state = st.copy()
        host_state["seq"] = seq
        if acc >= 0:
            host_x = x.copy()
    res = {"state": st, "rec": ops["rec"].copy(), "sums": sums, "x": x, "trial": ops["trial"].copy(), "dx_chain": ops["dx_chain"].copy(),
           "dx_acc": dx_acc, "partials": None if ops["partials"] is None else ops["partials"].copy(), "host_state": host_state,
           "host_x": host_x, "guard": -1}
    return res, path


def device(dtype, S, ops, **modes):
    """the same launch on the device"""
    modes.pop("plant", None)
    return api.lmDecide(ops["state"], ops["rec"], ops["sums"], ops["x"], ops["trial"], ops["dx_chain"], ops["dx_acc"], settings=S,
                        dtype=dtype, partials=ops["partials"], nparts=ops["nparts"], **modes)


# ---------------------------------------------------------------------------------------------------------------- assertions
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.dtype("u%d" % a.dtype.itemsize))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(bits(a), bits(b)))


STATE_ORDER = ["decision", "accepted_k", "consumed", "fcalls", "rejects", "guards", "qp_active", "null_tail", "coop_rescued", "spec_ok",
               "qp_status", "qp_iterations", "flags", "iterations", "seq"] + list(api.LM_STATE_FLOATS)


def compare_state(got, want, what="state"):
    for k in STATE_ORDER:
        assert same_bits(got[k], want[k]), "%s: %s %r, the reference %r" % (k, what, got[k][0], want[k][0])


def compare(got, want, mirror=True):
    """everything a launch returns against the reference, bit for bit; every assertion starts with the name of what differs"""
    assert got["guard"] == -1, "guard: band %d is damaged" % got["guard"]
    compare_state(got["state"], want["state"])
    for k in ("sums", "x", "dx_acc"):
        assert same_bits(got[k], want[k]), "%s: differs from the reference at %s" % (k, np.flatnonzero(bits(got[k]) != bits(want[k]))[:4])
    for k in ("rec", "trial", "dx_chain"):
        assert got[k].tobytes() == want[k].tobytes(), "%s: an input changed" % k
    if want["partials"] is not None:
        assert got["partials"].tobytes() == want["partials"].tobytes(), "partials: an input changed"
    compare_state(got["host_state"], want["host_state"], "mirror")
    assert same_bits(got["host_x"], want["host_x"]), "host_x: differs from the reference"
    if not mirror:
        assert set(got["host_state"].tobytes()) == {0xFF} and set(got["host_x"].tobytes()) == {0xFF}, "mirror: written without a mirror"


def untouched(got, ops, assigned):
    """every state field outside `assigned` keeps the bits it went in with"""
    for k in STATE_ORDER:
        if k not in assigned:
            assert same_bits(got["state"][k], ops["state"][k]), "%s: moved (%r -> %r)" % (k, ops["state"][k][0], got["state"][k][0])


ALWAYS = {"lambda", "mu", "residual", "qp_status", "qp_iterations", "flags", "decision", "iterations", "accepted_k", "consumed",
          "fcalls", "rejects", "guards", "qp_active", "null_tail", "coop_rescued", "spec_ok"}


def assigned_fields(path):
    """the state fields the walk assigns on a path (the others must keep their bits): by the D source, a pass that ends before
    LS:1115 has no trial residual, one that ends before LS:1124 no improvement, a rejection no step scalars, LS:1144 no rho"""
    a = set(ALWAYS)
    if any(p in path for p in ("reject", "not_finite", "no_prediction", "rate_poor", "rate_mid", "rate_good")):
        a.add("trial_residual")
    if any(p in path for p in ("reject", "no_prediction", "rate_poor", "rate_mid", "rate_good")):
        a.add("improvement")
    if any(p in path for p in ("no_prediction", "rate_poor", "rate_mid", "rate_good")):
        a |= {"dx_dot", "new_dx_dot", "predicted", "trial_xnorm"}
    if any(p in path for p in ("rate_poor", "rate_mid", "rate_good")):
        a.add("rho")
    return a


# ---------------------------------------------------------------------------------------------------------------- oracle replay
REPLAY = [("t3a", np.float64), ("t3a", np.float32), ("t3b", np.float64)]


def rho_stars(T, Sv):
    """a rho inside each of the three ranges of LS:1152-1161: half of minStepQuality, the middle of the two qualities, 1"""
    return {"rate_poor": Sv["minStepQuality"] * T(0.5), "rate_mid": (Sv["minStepQuality"] + Sv["goodStepQuality"]) / T(2), "rate_good": T(1)}


def oracle_rounds(name, dtype):
    """the oracle's trace of a problem under NON_DEFAULT, cut into rounds: the maximal runs of events 2 (rejected) and 4 (step guard),
    each closed by an event 3 (accepted) where there is one. A round: lambda, mu (tracked here: 1 after an acceptance or a forced
    refresh, doubled by a rejection and by a poor rating), residual and iterations before it, its events, the lambda of the
    event behind it (None at the end of the trace) and, for an acceptance, the rating that lambda shows."""
    import problems as P
    from oracle import oracle as O
    p = getattr(P, name)()
    S = O.default_settings(dtype)
    for k, v in _ND.items():
        setattr(S, k, v)
    T = dtype
    Sv = {k: T(getattr(S, k)) for k in SETTING_FIELDS}
    ev = []
    O.optimize(p["f"], p["m"], p["x0"], p["lower"], p["upper"], g=p["g"], settings=S, dtype=dtype,
               trace=lambda e, it, lam, res, tres, dxd: ev.append((e, it, dtype(lam), dtype(res), dtype(tres), dtype(dxd))))
    rounds, cur, mu, residual = [], None, T(1), None
    for i, (e, it, lam, res, tres, dxd) in enumerate(ev):
        nxt = ev[i + 1] if i + 1 < len(ev) else None
        if e in (0, 1):
            if e == 0 and mu > 16:                                                 # LS:984-989
                mu = T(1)
            residual = res
            continue
        if cur is None:
            cur = dict(lam=lam, mu=mu, residual=residual if e == 3 else res, iterations=it - 1 if e == 3 else it, events=[], outcome=None)
            lam_in = lam
        cur["events"].append((e, tres, dxd))
        if e in (2, 4):
            lam_in, mu = ref_reject(T, Sv, lam_in, mu)
        if e == 3 or nxt is None or nxt[0] in (0, 1):
            cur["next_lam"] = None if nxt is None else nxt[2]
            if e == 3:
                cur["accepted"] = (res, it)
                mu, residual = T(1), res
                cur["outcome"] = "rate_mid"
                if nxt is not None:
                    took = [o for o, rs in rho_stars(T, Sv).items() if same_bits(np.array(ref_rate(T, Sv, rs, lam_in, mu)[0]), np.array(nxt[2]))]
                    assert took, ("no rating explains the oracle's next lambda", cur)
                    cur["outcome"] = took[0]
                    mu = ref_rate(T, Sv, rho_stars(T, Sv)[took[0]], lam_in, mu)[1]
            rounds.append(cur)
            cur = None
    return rounds, S




def replay(decide, name, dtype):
    """feeds each round of the oracle's trace to `decide` (walk or device) as one chain; returns (rejections, good acceptances).
    For an acceptance predicted = improvement x rho*, rho* inside the range whose outcome the oracle's next lambda shows."""
    T = dtype
    rounds, So = oracle_rounds(name, dtype)
    S = settings_of(dtype, _ND)
    Sv = settings_values(S, T)
    assert all(T(getattr(So, k)) == Sv[k] for k in SETTING_FIELDS)
    rejections = good = 0
    for rd in rounds:
        evs, lam, mu = rd["events"], rd["lam"], rd["mu"]
        for c0 in range(0, len(evs), 8):                                           # a round longer than the ladder: in pieces
            part = evs[c0:c0 + 8]
            ops = build(["R"] * len(part), dtype, lam, mu, n=2)
            ops["state"]["residual"], ops["state"]["iterations"] = rd["residual"], rd["iterations"]
            for k, (e, tres, dxd) in enumerate(part):
                ops["rec"][k]["new_dx_dot"], ops["rec"][k]["flags"] = dxd, FLAG_GUARD if e == 4 else 0
                ops["sums"][k] = np.nan if e == 4 else tres
                rejections += e in (2, 4)
            if part[-1][0] == 3:
                improvement = T(rd["residual"]) - part[-1][1]
                ops["rec"][len(part) - 1]["predicted"] = improvement * rho_stars(T, Sv)[rd["outcome"]]
            got = decide(dtype, S, ops)
            if not isinstance(got, dict):
                got = got[0]
            st = got["state"]
            lam, mu = st["lambda"][0], st["mu"][0]
            if part[-1][0] == 3:
                assert st["decision"][0] == api.LM_DECIDE_ACCEPT and st["accepted_k"][0] == len(part) - 1, "decision: %r" % st
                assert same_bits(st["residual"], np.array([rd["accepted"][0]], dtype=dtype)) and st["iterations"][0] == rd["accepted"][1], "residual: %r" % st
                good += rd["outcome"] == "rate_good" and rd["next_lam"] is not None
            else:
                assert st["decision"][0] == api.LM_DECIDE_REJECT and st["rejects"][0] + st["guards"][0] == len(part), "decision: %r" % st
                assert same_bits(st["residual"], np.array([rd["residual"]], dtype=dtype)) and st["iterations"][0] == rd["iterations"], "residual: %r" % st
        if rd["next_lam"] is not None:
            assert same_bits(st["lambda"], np.array([rd["next_lam"]], dtype=dtype)), "lambda: %r, the oracle's next %r (round %r)" % (st["lambda"][0], rd["next_lam"], rd)
    assert rejections >= 3 and good >= 1, "the replay holds %d rejections and %d good acceptances: nothing is shown" % (rejections, good)
    return rejections, good
