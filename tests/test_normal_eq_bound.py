"""The order-independent fp64 bound of tests/ne_bound.py on the oracle's normal equations (orc.lm_step), at the parameter counts whose
tile edges the GPU tests exercise (tests/test_gpu_stage_calls.py): the reference the GPU is held to is itself checkable without a GPU."""
import numpy as np
import pytest

import ne_bound

H_INCR = float(np.sqrt(np.finfo(np.float32).eps))
# P = 6 (frames - 1): P + 1 = 31, 37, 61, 67, 97, 127, 193 -- a partial last 32-wide tile, 1 .. 7 tiles, the last P of the LDS kernel and
# the first of the matrix-core one; 198, 594, 1020, 1026: the first and last P of the panel solve, the loop-closure pass (P + 1 = 595, a
# last tile of 19 columns) and the first P of the host solve (tests/test_gpu_large_keyframe_sets.py)
P_LIST = [30, 36, 60, 66, 96, 126, 192, 198, 594, 1020, 1026]


def _system(rng, P, rows):
    """Residuals e0 and P forward-difference evaluations with the spread of magnitudes of a real batch: rows of very different size,
    columns that leave many rows exactly as they were (the Gaussians a pose does not touch), and a few extra rows (IMU / gravity /
    odometry) much larger than the rest."""
    e0 = rng.normal(0.0, 1.0, rows) * np.exp(rng.uniform(-6.0, 2.0, rows))
    J = rng.normal(0.0, 1.0, (P, rows)) * np.exp(rng.uniform(-4.0, 3.0, (P, 1)))
    J[rng.random((P, rows)) < 0.6] = 0.0
    e0[-5:] *= 1e3
    return e0, e0[None, :] + H_INCR * J


@pytest.mark.parametrize("P", P_LIST)
def test_oracle_normal_equations_within_fp64_bound(orc, P):
    rng = np.random.default_rng(P)
    lam = float(np.float32(1e-5))
    for rows in (P + 7, 777, 4096 + 300):  # fewer rows than a block, a few blocks, more than 16 blocks of 256
        e0, eb = _system(rng, P, rows)
        H, g, _ = orc.lm_step(e0, eb, H_INCR, lam, 0.2)
        assert ne_bound.check(H, g, lam, e0, eb, H_INCR) <= 1.0


def test_bound_catches_a_wrong_tile_and_a_dropped_block(orc):
    """The bound has teeth: H with one row block left out, or one off-diagonal 32 x 32 tile taken from the wrong place, fails it."""
    rng = np.random.default_rng(1)
    P, rows = 66, 1100
    lam = float(np.float32(1e-5))
    e0, eb = _system(rng, P, rows)
    H, g, _ = orc.lm_step(e0, eb, H_INCR, lam, 0.2)
    assert ne_bound.check(H, g, lam, e0, eb, H_INCR) <= 1.0
    J = ne_bound.jacobian(e0, eb, H_INCR)
    blk = J[256:512]
    H_drop = H - blk.T @ blk
    with pytest.raises(AssertionError, match="H outside"):
        ne_bound.check(H_drop, g, lam, e0, eb, H_INCR)
    H_tile = H.copy()
    H_tile[0:32, 32:64] = H[32:64, 0:32]  # the mirror of a tile written un-transposed
    with pytest.raises(AssertionError, match="H outside"):
        ne_bound.check(H_tile, g, lam, e0, eb, H_INCR)
    g_drop = g - J[-5:].T @ e0[-5:]  # the additional rows left out of g
    with pytest.raises(AssertionError, match="g outside"):
        ne_bound.check(H, g_drop, lam, e0, eb, H_INCR)
