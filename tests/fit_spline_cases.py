"""Inputs shared by tests/test_fit_spline_gpu_host.py and tests/test_gpu_fit_spline.py (fitSpline on device-resident points).
Everything is generated from fixed seeds; nothing here needs a GPU."""
import numpy as np

import mir_optim_amd as M

# fit_splie.d:94-137: the reference's unittest data and expected spline values, restated as data
X = np.array([-1.0, 2, 4, 5, 8, 10, 12, 15, 19, 22])
Y0 = np.array([17.0, 0, 16, 4, 10, 15, 19, 5, 18, 6])
POINTS = np.column_stack([X + 0.5, [-0.68361541, 7.28568719, 10.490694, 0.36192032, 11.91572713, 16.44546433,
                                   17.66699525, 4.52730869, 19.22825394, -2.3242592]])
Y_LAMBDA = np.array([15.898984945597563, 0.44978154774119194, 15.579636654078188, 4.028312405287987, 9.945895290402778,
                     15.07778815727665, 18.877926155854535, 5.348699237978274, 16.898507797404278, 22.024920998359942])
APPROX = 2.0 ** -20         # mir.test shouldApprox: maxRelDiff = maxAbsDiff = 0x1p-20


def approx(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(np.abs(a - b) <= APPROX * np.maximum(np.abs(a), np.abs(b)) + APPROX))


FAMILIES = ("uniform", "alternating", "pivoting")


def knots(nx, family):
    """uniform: random spacings in [0.3, 2.0); alternating: spacings 0.02 / 1.0 in turn; pivoting: spacings 0.02, 0.02, 1.0 in
    turn. The elimination of the not-a-knot system exchanges rows i and i + 1 when |lo[i + 1]| > |di[i]|. After step 0
    (multiplier exactly 1) di[1] = h0 + h1, so step 1 exchanges when h2 > h0 + h1; a later step needs h[i + 1] > 2 h[i - 1] +
    4/3 h[i] or so. Spacings that merely alternate never get there (h2 = h0), two short intervals before a long one do:
    test_pivoting_knots_pivot holds the third family to at least one exchange, and records that the second makes none."""
    if family == "uniform":
        return np.cumsum(np.random.default_rng(1000 + nx).uniform(0.3, 2.0, nx))
    if family == "alternating":
        return np.cumsum(np.where(np.arange(nx) % 2 == 0, 0.02, 1.0))
    return np.cumsum(np.where(np.arange(nx) % 3 == 2, 1.0, 0.02))


def abscissae(x, seed):
    """Three uniform points inside every knot interval, every knot itself, two points below x[0] and two above x[-1],
    shuffled."""
    rng = np.random.default_rng(seed)
    parts = [x.copy(), x[0] - rng.uniform(0.1, 1.5, 2), x[-1] + rng.uniform(0.1, 1.5, 2)]
    for a, b in zip(x[:-1], x[1:]):
        parts.append(rng.uniform(a, b, 3))
    t = np.concatenate(parts)
    rng.shuffle(t)
    return t


def smooth(t):
    return 3.0 * np.sin(0.7 * t) + 0.1 * t


def points_for(x, seed, count=None):
    """count points {t, smooth(t) + N(0, 0.1)} at the abscissae above (repeated in turn when count exceeds them)."""
    t = abscissae(x, seed)
    if count is not None:
        t = np.resize(t, count)
    rng = np.random.default_rng(seed + 7)
    return np.column_stack([t, smooth(t) + rng.normal(0.0, 0.1, t.size)])


# ---- the callback-level grid
GRID_NX = (1, 2, 3, 4, 5, 10, 37, 64, 65, 128)
GRID_LAMBDA = (0.0, 1e-3)
GRID_NP = (1, 63, 64, 65, 257)


def grid_cases(nx, family):
    """(lambda, points, X) of one knot vector: every lambda, every point count (clipped to >= nx where lambda == 0, as the
    entry demands) and both p = 2 nx and p = 2 nx + 1 random value vectors."""
    x = knots(nx, family)
    out = []
    for lam in GRID_LAMBDA:
        counts = sorted({max(c, nx) if lam == 0 else c for c in GRID_NP})
        for c in counts:
            pts = points_for(x, 31 * nx + c, c)
            for p in (2 * nx, 2 * nx + 1):
                rng = np.random.default_rng(nx * 1000 + c + p)
                out.append((lam, pts, rng.normal(0.0, 2.0, (p, nx))))
    return x, out


def reference_residuals(points, x, lam, V):
    """fit_spline.cpp's residual function, one vector at a time (double)."""
    return np.stack([M.fit_spline_residuals(points, x, lam, v) for v in V])


def reference_residuals_f32(points, x, lam, V):
    """The same function as a FLOAT run of fit_spline.cpp: its derivatives (mir_spline_c2_derivatives_s), its evaluation
    (mir_spline_eval_s) and the penalty of its lines 123-132 in numpy float32 scalars (every + * / sqrt rounded to float)."""
    f = np.float32
    points = np.asarray(points, dtype=f)
    x = np.asarray(x, dtype=f)
    k, nx = points.shape[0], x.size
    m = k + (1 if lam == 0 else 0)
    out = np.zeros((len(V), m), dtype=f)
    for r, v in enumerate(np.asarray(V, dtype=f)):
        s = M.Spline(x, v, np.float32)
        for i in range(min(k, m)):
            out[r, i] = s.withTwoDerivatives(points[i, 0])[0] - points[i, 1]
        integral = f(0)
        if lam != 0:
            d = s.derivatives
            ld = d[0]
            for i in range(1, nx):
                rd = d[i]
                integral = integral + (rd * rd + rd * ld + ld * ld) * (x[i] - x[i - 1])
                ld = rd
        out[r, m - 1] = np.sqrt(integral * f(lam) * f(k) / f(3 * nx))
    return out


# ---- the fit-level inputs: (name, points, knots, lambda, lower, upper)
def fit_cases():
    inf10 = np.full(10, np.inf)
    cases = [("reference-0", POINTS, X, 0.0, -inf10, inf10), ("reference-lambda", POINTS, X, 1e-3, -inf10, inf10),
             ("reference-box", POINTS, X, 1e-3, np.zeros(10), np.full(10, 15.0))]
    return cases + generated_cases()


def generated_cases():
    out = []
    x4 = knots(4, "uniform")
    out.append(("nx4-np4", points_for(x4, 404)[:4], x4, 0.0))
    for family in FAMILIES:
        x37 = knots(37, family)
        for lam in (0.0, 1e-2):
            out.append((f"nx37-{family}-{lam}", points_for(x37, 3700), x37, lam))
    x130 = knots(130, "uniform")
    out.append(("nx130", points_for(x130, 13000), x130, 1e-2))
    return [(name, pts, x, lam, np.full(x.size, -np.inf), np.full(x.size, np.inf)) for name, pts, x, lam in out]
