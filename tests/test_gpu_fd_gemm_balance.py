"""Forked difference-panel GEMM at n = 128 (workloads_gemm.hip, tlb_fork_*) after the base chain moved to the four-block
4x4x4 f64 MFMA, the group -> wave assignment became a table that the structure check reads too, and the steady-state epilogue
lost its row compares: the default entry must still give the bits of the dense entry
  * at row counts around one tile, one 32-row stage, and where some workgroups of the 256-workgroup grid run one stage more than
    others and the last stage is partial (the row-compare-free epilogue must never run on a partial stage);
  * on X that breaks the finite-difference structure by one ulp at the last coordinate a group takes from the base chain
    (coordinate 8 g - 1 for group g: the check must send the call to the dense GEMM), and at the first coordinate that the
    group multiplies itself (8 g: the check passes and the forked chain must use the changed value), for every group."""
import numpy as np
import pytest

from test_gpu_fd_prefix_gemm import both_panels, fd_points, mixed_point, same_bits

pytestmark = pytest.mark.gpu

N = 128


@pytest.mark.parametrize("m", [1, 15, 16, 17, 31, 32, 33, 63, 65, 32 * 256 + 33, 32 * 256 * 2 + 17])
def test_forked_panel_equals_dense_panel(m):
    x, lower, upper = mixed_point(N, 1000 + m % 89)
    X = fd_points(x, lower, upper, 2.0 ** -20)
    w, (Df, Dd) = both_panels(m, N, X)
    assert same_bits(Df, Dd)
    y = np.tanh(w["A"] @ X.T) - w["b"][:, None]
    ref = y[:, 0::2] - y[:, 1::2]
    assert np.allclose(Df, ref, rtol=0, atol=1e-12)
    assert np.all(Df[:, 5] == 0.0)
    assert np.abs(Df).max() > 0 or np.abs(ref).max() < 1e-9     # (a single row can saturate tanh: all differences zero)


@pytest.mark.parametrize("g", range(1, 16))
def test_one_ulp_at_each_groups_fork_boundary_equals_dense(g):
    m = 32 * 256 + 33
    x, lower, upper = mixed_point(N, 7)
    for k in (8 * g - 1, 8 * g):
        for p in (16 * g, 16 * g + 15):                  # first and last point of the group; their own coordinates are p // 2
            X = fd_points(x, lower, upper, 2.0 ** -20)
            X[p, k] = np.nextafter(X[p, k], np.inf)
            _, (Df, Dd) = both_panels(m, N, X)
            assert same_bits(Df, Dd), (g, p, k)
