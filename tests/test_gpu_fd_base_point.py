"""MIR_LSQ_FD_BASE_POINT: a fbRowMajorDiff callback that also takes p = 2n + 1 -- the m x n difference panel of the first 2n points
and, behind it, the residual vector of one more point. The library then makes the entry residual f(x0) and the first refresh's
panel in one call (Solver::fd_entry); at n = 128 the caller's GEMM (workloads_gemm.hip, the BASE instance) forms that residual
from the stage of A it holds in LDS, with the arithmetic of the one-point sweep.

Callback level: p = 2n + 1 against two separate calls (p = 2n, and wl_tanh_linear_f_d on the last point), bit for bit, for both
entries, forked and dense, partial stages, the shapes that fall back to the one-point kernel, and a canary behind everything.
Solve level: the flag against MIR_LSQ_VARIANT_NO_FD_BASE_POINT -- x, every result field, every counter and the trace are equal,
and a counting trampoline sees exactly one p = 2n + 1 call, at entry, and one f call fewer."""
import ctypes as C

import numpy as np
import pytest

import mir_optim_amd as M
from mir_optim_amd import api, parallel, workloads as W
import problems as P

pytestmark = pytest.mark.gpu

F_T = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p)
FB_T = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p)
ENTRIES = ("wl_tanh_linear_fbd_d", "wl_tanh_linear_fbd_dense_d")
CANARY = -12345.678
_problems = {}


def problem(m, n):
    """one data set and device problem per shape, shared by the tests and left unchanged"""
    if (m, n) not in _problems:
        w = P.tanh_linear(m, n)
        _problems[(m, n)] = (w, W.TanhLinear(w["A"], w["b"]))
    return _problems[(m, n)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def fd_points(x, eps=2.0 ** -20):
    n = x.size
    X = np.repeat(x[None, :], 2 * n, axis=0)
    j = np.arange(n)
    X[2 * j, j] = x + eps
    X[2 * j + 1, j] = x - eps
    return X


def call_entry(prob, entry, m, n, p, X, out_len):
    dX = api.DeviceBuffer(np.ascontiguousarray(X))
    dD = api.DeviceBuffer(np.full(out_len, CANARY))
    getattr(api.workloads_lib(), entry)(C.c_void_p(C.addressof(prob.ctx)), C.c_size_t(m), C.c_size_t(n), C.c_size_t(p),
                                        C.c_void_p(dX.ptr), C.c_void_p(dD.ptr))
    prob.stream.synchronize()
    out = dD.download()
    dX.free()
    dD.free()
    return out


def one_point(prob, m, n, x):
    dx = api.DeviceBuffer(np.ascontiguousarray(x))
    dy = api.DeviceBuffer(np.full(m, CANARY))
    api.workloads_lib().wl_tanh_linear_f_d(C.c_void_p(C.addressof(prob.ctx)), C.c_size_t(m), C.c_size_t(n), C.c_void_p(dx.ptr),
                                           C.c_void_p(dy.ptr))
    prob.stream.synchronize()
    y = dy.download()
    dx.free()
    dy.free()
    return y


# n = 128: less than one stage, exactly one, a one-row partial stage, 256 workgroups with a second stage on some and a partial last
# one; the other n: the panel kernel of that shape, then the one-point kernel for the last point
SHAPES = [(7, 128), (32, 128), (33, 128), (8293, 128), (8293, 16), (8293, 64), (8293, 126), (8293, 192)]


@pytest.mark.parametrize("kind", ["base", "foreign", "far"])
@pytest.mark.parametrize("m,n", SHAPES)
def test_panel_and_extra_point_equal_two_separate_calls(m, n, kind):
    w, prob = problem(m, n)
    x = w["x0"].copy()
    X = np.empty((2 * n + 1, n))
    X[:2 * n] = fd_points(x)
    X[2 * n] = x
    if kind == "foreign":                      # one finite-difference point altered in a coordinate not its own: the vote fails
        X[2 * n - 1, 0] = np.nextafter(X[2 * n - 1, 0], np.inf)
    if kind == "far":                          # "one more point", not "the base"
        X[2 * n] = -3.0 * x + np.linspace(-2.0, 2.0, n)
    y_ref = one_point(prob, m, n, X[2 * n])
    assert not np.any(y_ref == CANARY) and np.allclose(y_ref, np.tanh(w["A"] @ X[2 * n]) - w["b"], rtol=0, atol=1e-13)
    for entry in ENTRIES:
        ref = call_entry(prob, entry, m, n, 2 * n, X[:2 * n], m * n + m + 16)
        assert np.all(ref[m * n:] == CANARY)   # p = 2n: nothing is written past the panel
        got = call_entry(prob, entry, m, n, 2 * n + 1, X, m * n + m + 16)
        assert np.array_equal(bits(got[:m * n]), bits(ref[:m * n])), entry
        assert np.array_equal(bits(got[m * n:m * n + m]), bits(y_ref)), entry
        assert np.all(got[m * n + m:] == CANARY)


# ---- whole solves ----------------------------------------------------------------------------------------------------------------

def counters(st):
    return {k: v for k, v in st.as_dict().items() if not k.endswith("_ms")}


def solve(prob, w, variant=0, log=None, **kw):
    """One solve; log: a list that receives ('f',) and ('fbd', p) in call order through counting trampolines."""
    keep = []
    saved = prob.f, prob.fbd
    if log is not None:
        nf, nfbd = F_T(prob.f), FB_T(prob.fbd)

        def f_tr(ctx, m, n, x, y):
            log.append(("f",))
            nf(ctx, m, n, x, y)

        def fbd_tr(ctx, m, n, p, X, Y):
            log.append(("fbd", int(p)))
            nfbd(ctx, m, n, p, X, Y)
        keep = [F_T(f_tr), FB_T(fbd_tr)]
        prob.f = C.cast(keep[0], C.c_void_p).value
        prob.fbd = C.cast(keep[1], C.c_void_p).value
    try:
        st = M.Stats()
        s = kw.pop("settings", None)
        if s is None:
            s = M.LeastSquaresSettings(); s.absTolerance = 1e-9
        trace = api.Trace(512) if kw.pop("trace", False) else None
        res, x = prob.solve(kw.pop("x0", w["x0"]), settings=s, batched=kw.pop("batched", True), stats=st, variant=variant,
                            trace=trace, **kw)
    finally:
        prob.f, prob.fbd = saved
    fields = (int(res.status), res.iterations, res.fCalls, res.gCalls, bits([res.residual])[0], bits([res.lambda_])[0])
    return fields, x, counters(st), trace.records() if trace else None


def assert_same_solve(a, b):
    assert a[0] == b[0]
    assert np.array_equal(bits(a[1]), bits(b[1]))
    assert a[2] == b[2]
    assert a[3] == b[3]


@pytest.mark.parametrize("flow", ["fused", "no_pipeline", "trace", "one_rank", "bounds"])
@pytest.mark.parametrize("m,n", [(8293, 128), (2000, 16)])
def test_solve_with_the_flag_equals_solve_without(m, n, flow):
    w, prob = problem(m, n)
    variant = api.VARIANT_NO_PIPELINE if flow == "no_pipeline" else 0
    kw = {}
    if flow == "trace":
        kw["trace"] = True
    if flow == "bounds":
        lo, up = np.full(n, -np.inf), np.full(n, np.inf)
        lo[3] = up[3] = w["x0"][3]                                   # collapsed interval: twh = 0
        lo[5] = w["x0"][5] - 2.0 ** -30                              # clips x - h
        up[n - 1] = w["x0"][n - 1] + 2.0 ** -30                      # clips x + h
        kw["l"], kw["u"] = lo, up
    comm = parallel.HostAllreduceComm(1, 0, lambda buf: None) if flow == "one_rank" else None
    try:
        if comm:
            kw["comm"] = comm
        log_on, log_off = [], []
        on = solve(prob, w, variant, log_on, **dict(kw))
        off = solve(prob, w, variant | api.VARIANT_NO_FD_BASE_POINT, log_off, **dict(kw))
    finally:
        if comm:
            comm.close()
    assert on[0][0] >= 0 and on[2]["jacobian_full"] >= 1
    assert_same_solve(on, off)
    # exactly one fbd call with p = 2n + 1, the first callback of the solve; every other refresh with p = 2n; one f call fewer
    assert log_on[0] == ("fbd", 2 * n + 1) and log_off[0] == ("f",)
    assert [e for e in log_on[1:] if e[0] == "fbd"] == [("fbd", 2 * n)] * (on[2]["jacobian_full"] - 1)
    assert [e for e in log_off if e[0] == "fbd"] == [("fbd", 2 * n)] * off[2]["jacobian_full"]
    assert log_on.count(("f",)) == log_off.count(("f",)) - 1
    # the early k_fd_points is booked to the first refresh round: the entry keeps its three launches (a flush of the pending
    # Broyden terms belongs to no round either, tests/test_gpu_launch_budget.py)
    if on[2]["broyden_flushes"] == 0:
        assert on[2]["library_launches"] == sum(on[2]["round_launches"]) + 3


@pytest.mark.parametrize("m,n", [(8293, 128), (2000, 16)])
def test_entry_residual_that_converges_discards_the_panel(m, n):
    w, prob = problem(m, n)
    outs = []
    for variant in (0, api.VARIANT_NO_FD_BASE_POINT):
        # the entry residual satisfies fConverged (LS:956: residual <= maxGoodResidual -- the setting that test reads here;
        # a large absTolerance alone ends such a solve with xConverged after a refresh)
        s = M.LeastSquaresSettings(); s.absTolerance = 1e30; s.maxGoodResidual = 1e30
        log = []
        outs.append(solve(prob, w, variant, log, settings=s) + (log,))
    on, off = outs
    assert on[0][0] == int(M.LeastSquaresStatus.fConverged) and on[0][2] == 1            # status, fCalls
    assert_same_solve(on[:4], off[:4])
    assert on[4] == [("fbd", 2 * n + 1)] and off[4] == [("f",)]                        # the documented difference
    assert on[2]["fd_callback_calls"] == 0 and on[2]["fd_callback_points"] == 0 and on[2]["library_launches"] == 3


@pytest.mark.parametrize("case", ["analytic", "separate_fill", "pair_panel", "point_major"])
def test_paths_that_keep_their_own_entry_residual(case):
    m, n = 2000, 16
    w, prob = problem(m, n)
    kw = {"analytic": True} if case == "analytic" else {}
    if case == "pair_panel":
        kw["batched"] = "rowmajor"
    if case == "point_major":
        kw["batched"] = "pointmajor"
    variant = api.VARIANT_FD_SEPARATE_FILL if case == "separate_fill" else 0
    log_on, log_off = [], []
    on = solve(prob, w, variant, log_on, flags=api.FD_BASE_POINT, **dict(kw))
    off = solve(prob, w, variant | api.VARIANT_NO_FD_BASE_POINT, log_off, **dict(kw))
    assert on[0][0] >= 0
    assert_same_solve(on, off)
    assert log_on == log_off and log_on[0] == ("f",) and all(e[0] == "f" for e in log_on)


def test_host_callbacks_ignore_the_flag():
    m, n = 2000, 16
    w, _ = problem(m, n)
    A, b = w["A"], w["b"]

    def f(x, y):
        y[:] = np.tanh(A @ x) - b
    seen = []
    tramp = FB_T(lambda *a: seen.append(a[3]))
    outs = []
    for flags in (api.FD_BASE_POINT, 0):
        o = api.GpuOptions()
        o.flags = flags
        o.fbRowMajorDiff = C.cast(tramp, C.c_void_p).value
        s = M.LeastSquaresSettings(); s.absTolerance = 1e-9
        res, x = api.optimizeLeastSquares(f, m, w["x0"].copy(), settings=s, options=o)
        outs.append(((int(res.status), res.iterations, res.fCalls, bits([res.residual])[0]), x))
    assert outs[0][0] == outs[1][0] and outs[0][0][0] >= 0 and np.array_equal(bits(outs[0][1]), bits(outs[1][1]))
    assert seen == []


def test_repeated_solves_on_one_workspace_are_bit_identical():
    m, n = 8293, 128
    w, prob = problem(m, n)
    ws = api.lib().mir_lsq_workspace_create(C.c_size_t(m), C.c_size_t(n), C.c_size_t(8))
    assert ws
    try:
        runs = [solve(prob, w, v, workspace=ws) for v in (0, 0, api.VARIANT_NO_FD_BASE_POINT, 0)]
    finally:
        api.lib().mir_lsq_workspace_destroy(C.c_void_p(ws))
    for r in runs[1:]:
        assert_same_solve(runs[0], r)
