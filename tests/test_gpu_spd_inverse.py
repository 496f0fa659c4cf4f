"""The SPD inverse on the device (csrc/spd_inverse.h through mir_lsq_spd_inverse_* / M.spdInverse) against numpy in float64.

Inputs: P = Q diag(lambda) Q^T with a geometric spectrum of condition 1e3 (spd() below, as tests/test_gpu_big_n.py builds
it). Two figures per case: err = max|X - inv(P)| / max|inv(P)| and the normalised residual
nres = ||P X - I||_F / (||P||_F ||X||_F).

Measured on an MI355X (profiles/r09/covariance.txt), the largest value over the sizes of a precision, the equilibration and the
fixed-mask cases included:
    f64: err 4.328e-14 (n = 1024), nres 8.184e-17   (numpy.linalg.inv itself: nres up to 3.291e-17)
    f32: err 2.213e-05,            nres 2.591e-08
The tolerances below are 8 x these values. The panel of the factorization is 16 columns wide: 15, 16, 17, 31 and 33 are in the
size list."""
import functools

import numpy as np
import pytest

import mir_optim_amd as M

pytestmark = pytest.mark.gpu

TOL_ERR = {np.float64: 8 * 4.328e-14, np.float32: 8 * 2.213e-05}
TOL_NRES = {np.float64: 8 * 8.184e-17, np.float32: 8 * 2.591e-08}
SIZES64 = [1, 2, 3, 7, 8, 15, 16, 17, 31, 33, 64, 65, 128, 129, 200, 256, 257, 300, 1024]
SIZES32 = [1, 8, 17, 128, 129, 300]
EPS64 = np.finfo(np.float64).eps


def spd(n, seed, cond=1e3):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.geomspace(1.0, cond, n)
    return (Q * d) @ Q.T


@functools.lru_cache(maxsize=None)
def case(n):
    """(P, inv(P) by numpy, numpy's own normalised residual), float64, computed once"""
    P = spd(n, n)
    Xr = np.linalg.inv(P)
    for a in (P, Xr):
        a.setflags(write=False)
    return P, Xr, nres(P, Xr)


def nres(P, X):
    P, X = np.asarray(P, dtype=np.float64), np.asarray(X, dtype=np.float64)
    return np.linalg.norm(P @ X - np.eye(len(P))) / (np.linalg.norm(P) * np.linalg.norm(X))


def err(X, Xr):
    return np.abs(np.asarray(X, dtype=np.float64) - Xr).max() / np.abs(Xr).max()


@pytest.mark.parametrize("dtype,n", [(np.float64, n) for n in SIZES64] + [(np.float32, n) for n in SIZES32])
def test_inverse_matches_numpy(dtype, n):
    P, Xr, np_res = case(n)
    Pd = P.astype(dtype)
    X, info = M.spdInverse(Pd, dtype=dtype)
    assert info == 0 and X.dtype == dtype and X.shape == (n, n)
    assert np.array_equal(X, X.T)                                        # symmetric to the bit
    X2, info2 = M.spdInverse(Pd, dtype=dtype)
    assert info2 == 0 and np.array_equal(X, X2)                          # the same bits again
    e, r = err(X, Xr), nres(Pd, X)
    print(f"spd_inverse {np.dtype(dtype).name} n={n}: err {e:.3e} nres {r:.3e} (numpy nres {np_res:.3e})")
    assert e <= TOL_ERR[dtype] and r <= TOL_NRES[dtype]
    if dtype == np.float64:
        # sanity, not a tolerance: within 16 x numpy's own residual (which can be exactly 0 at n = 1: floored at one eps)
        assert r <= 16 * max(np_res, EPS64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [17, 129])
def test_badly_scaled_rows_keep_their_accuracy(dtype, n):
    """D P D with D = diag(10^k), k spread over -6 .. 6: without the ?poequ / ?laqsy step the small rows are lost. Compared
    after scaling back: D X D against inv(P)."""
    P, Xr, _ = case(n)
    d = 10.0 ** np.linspace(-6, 6, n)
    np.random.default_rng(n).shuffle(d)
    Ps = (P * np.outer(d, d)).astype(dtype)
    X, info = M.spdInverse(Ps, dtype=dtype)
    assert info == 0 and np.array_equal(X, X.T)
    Xb = X.astype(np.float64) * np.outer(d, d)
    e, r = err(Xb, Xr), nres(P, Xb)
    print(f"spd_inverse {np.dtype(dtype).name} n={n} scaled: err {e:.3e} nres {r:.3e}")
    assert e <= TOL_ERR[dtype] and r <= TOL_NRES[dtype]


@pytest.mark.parametrize("n", [17, 129])
def test_not_positive_definite(n):
    P, _, _ = case(n)
    for k in (0, n // 2, n - 1):
        for bad in (-P[k, k], np.nan):
            Q = P.copy()
            Q[k, k] = bad
            X, info = M.spdInverse(Q)
            assert info == k + 1 and np.all(np.isposinf(X)), (k, bad)
    # a NaN below the diagonal reaches the pivot of its row
    Q = P.copy()
    Q[n // 2, 1] = np.nan
    X, info = M.spdInverse(Q)
    assert info == n // 2 + 1 and np.all(np.isposinf(X))
    Xf, info = M.spdInverse(Q.astype(np.float32), dtype=np.float32)
    assert info == n // 2 + 1 and np.all(np.isposinf(Xf))
    # among the FREE indices: with index 0 fixed the failing minor of index k is minor k
    Q = P.copy()
    Q[3, 3] = -1.0
    fixed = np.zeros(n, dtype=bool); fixed[0] = True
    X, info = M.spdInverse(Q, fixed=fixed)
    assert info == 3
    assert np.all(X[0] == 0) and np.all(X[:, 0] == 0) and np.all(np.isposinf(X[1:, 1:]))


def fixed_sets(n):
    return {"first": [0], "middle": [n // 2], "last": [n - 1], "three": [0, n // 2, n - 1], "all_but_one": [i for i in range(n) if i != 1]}


@pytest.mark.parametrize("which", ["first", "middle", "last", "three", "all_but_one"])
@pytest.mark.parametrize("n", [17, 129])
def test_fixed_mask(n, which):
    P, _, _ = case(n)
    fx = np.zeros(n, dtype=bool)
    fx[fixed_sets(n)[which]] = True
    free = np.flatnonzero(~fx)
    Q = P.copy()
    Q[fx, :] = np.nan                                                   # proof that fixed rows and columns are not read
    Q[:, fx] = np.nan
    X, info = M.spdInverse(Q, fixed=fx)
    assert info == 0 and np.array_equal(X, X.T)
    assert np.all(X[fx, :] == 0) and np.all(X[:, fx] == 0)
    Pr = P[np.ix_(free, free)]
    Xr, info_r = M.spdInverse(Pr)
    assert info_r == 0
    Xn = np.linalg.inv(Pr)
    e, r = err(X[np.ix_(free, free)], Xn), nres(Pr, X[np.ix_(free, free)])
    print(f"spd_inverse fixed n={n} {which}: err {e:.3e} nres {r:.3e}; vs the reduced call {err(X[np.ix_(free, free)], Xr):.3e}")
    assert err(X[np.ix_(free, free)], Xr) <= TOL_ERR[np.float64]
    assert e <= TOL_ERR[np.float64] and r <= TOL_NRES[np.float64]
