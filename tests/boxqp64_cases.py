"""What the tests of the batched box-constrained QP solves of order 17 .. 64 share (tests/test_batched_boxqp64_host.py on the
CPU, tests/test_gpu_batched_boxqp64.py on the device): the orders, the 64-problem families of tests/boxqp_cases.py with the
one-problem entry's margin screen, and a wrapper of M.solveBoxQPBatchedWide that hands P in as its lower triangle with NaN
above (QP:109). Nothing here needs a device but a call of solve."""
import numpy as np

import mir_optim_amd as M
import boxqp_cases as B

NS_W32 = (17, 31, 32)                  # k_boxqp_wave<32, T>, two problems a wave: the first order, one short of full, full
NS_W64 = (33, 63, 64)                  # k_boxqp_wave<64, T>, one problem a wave
NS64 = NS_W32 + NS_W64
COUNT = 64
MAX_SCREENED_OUT = 2                   # problems of COUNT, per order and precision, at SINGLE_MARGIN
GRID_WAVES = 8192                      # kBoxQpMaxWaves of csrc/boxqp_launch.h


def problems_per_wave(n):
    return 2 if n <= 32 else 1


def fam(n, dtype):
    return B.family(n, dtype, count=COUNT)


def oracles(oracle, n, dtype):
    """(the same-precision oracle's, the f64 oracle's) answers on fam(n, dtype), computed once and shared"""
    return B.oracle_family(oracle, n, dtype, count=COUNT), B.oracle_family(oracle, n, np.float64, dtype, COUNT)


def screen(oracle, n, dtype):
    return B.screen_family(oracle, n, dtype, B.SINGLE_MARGIN[dtype], COUNT)


def solve(P, q, l, u, dtype, **kw):
    st, x, it = M.solveBoxQPBatchedWide(B.lower_only(np.asarray(P)), q, l, u, dtype=dtype, **kw)
    assert x.dtype == dtype and st.shape == it.shape == (len(q),) and x.shape == np.shape(q)
    return st, x, it


def class0(found, n):
    """the class-0 member of a mixed wave, as the n = 16 tests build it: the class-1 problem with bounds +-1e3"""
    P, q, _, _ = found[1]
    return P, q, np.full(n, -1e3), np.full(n, 1e3)
