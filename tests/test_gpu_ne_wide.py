"""The normal equations above 64 parameters and the line search's squared sums on caller data (hooks dmsa_debug_normal_equations and
dmsa_debug_squared_sums): k_jacobian_columns forms the columns in place, k_normal_eq_mfma contracts them on the matrix cores (64-row panels, a
chained v_mfma_f64_16x16x4_f64, mirrored tiles), k_normal_eq_reduce adds the block sums sixteen at a time plus a tail, ne_rows_per_split sizes
the blocks; k_squared_sums_blocked sums 1024-row chunks per block, fused above 64 parameters.  Whole calls reach these only at the row counts
a scene happens to give (tests/test_gpu_large_keyframe_sets.py).  Everything compares bit patterns -- with the oracle's export of its
blocked_dot on the whole result and with the exact chain of tests/ne_wide_cases.py on a sample -- except the order-independent bound of
tests/ne_bound.py on one case per size."""
import numpy as np
import pytest

import ne_bound
import ne_wide_cases as nw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def opt(hip):
    o = hip.DmsaOptimizer()
    yield o
    o.close()


@pytest.mark.parametrize("P,rows", nw.NE_CASES)
def test_normal_equations_above_64_parameters(opt, orc, P, rows):
    """formed = 0: the residual batch, columns formed on the device; formed = 1: the batch that holds the same columns already -- one reference"""
    E = nw.batch(P, rows)
    A = nw.columns(E, nw.H_STEP, False)
    ref, sample = orc.blocked_gram(A, P), nw.fused_sample(A, P)
    for formed, Ein in ((False, E), (True, nw.formed_batch(E, nw.H_STEP))):
        before = Ein.copy()
        Hp = opt.normalEquationsOf(Ein, nw.H_STEP, formed)
        assert np.array_equal(nw.bits(Ein), nw.bits(before)), "the caller's batch was written"
        differing = np.argwhere(nw.bits(Hp) != nw.bits(ref))
        assert differing.size == 0, (P, rows, formed, f"{len(differing)} elements differ from the oracle's order, first {differing[:5].tolist()}")
        assert np.array_equal(nw.bits(Hp), nw.bits(Hp.T)), (P, rows, formed, "mirror")
        nw.check_sample(Hp, sample, (P, rows, formed))
        if rows == nw.NE_BOUND_ROWS and not formed:
            worst = ne_bound.check(Hp[:P, :P], Hp[:P, P], 0.0, E[0], E[1:], nw.H_STEP)
            print(f"[ne_wide] P={P} rows={rows}: worst |error| / bound = {worst:.3f}")
            assert worst <= 1.0


@pytest.mark.parametrize("name", sorted(nw.SPECIAL))
@pytest.mark.parametrize("where", ["e0", "column"])
def test_special_values_above_64_parameters(opt, orc, name, where):
    """NaN, inf, -0.0, one denormal entry, and a whole evaluation of ~1e-160 whose products and sums are denormal: the matrix-core chain
    against std::fma (the oracle) and against the exact chain, non-NaN bits and NaN positions"""
    for P, rows in nw.SPECIAL_SHAPES:
        E = nw.special_batch(P, rows, name, where)
        for formed in (False, True):
            A = nw.columns(E, 0.5, formed)
            Hp = opt.normalEquationsOf(E, 0.5, formed)
            nw.same_bits_or_nan(Hp, orc.blocked_gram(A, P), (name, where, P, rows, formed))
            nw.check_sample(Hp, nw.fused_sample(A, P), (name, where, P, rows, formed))
            if name in ("nan", "inf"):
                assert np.isnan(Hp).any() or np.isinf(Hp).any()
            if name == "tiny" and (formed or where == "e0"):
                c = P if where == "e0" else P - 31
                assert 0.0 < Hp[c, c] < 2.3e-308, Hp[c, c]  # a denormal sum of denormal products, not flushed


@pytest.mark.parametrize("B,P,rows", nw.SQ_CASES)
def test_squared_sums(opt, orc, B, P, rows):
    """P = 64: 256-row blocks, a rounded square and a rounded sum per row; P = 65: the blocks of the rule, one fused multiply-add per row"""
    for kind in ("random", "cancellation"):
        E = nw.squares_input(B, rows, kind)
        got = opt.squaredSumsOf(E, P)
        model = nw.fused_squares(E, P) if P > 64 else nw.unfused_squares(E, nw.reduction_block_rows(rows, P))
        assert np.array_equal(nw.bits(got), nw.bits(model)), (B, P, rows, kind, "model", got[:3], model[:3])
        assert np.array_equal(nw.bits(got), nw.bits(orc.blocked_squares(E, P))), (B, P, rows, kind, "oracle")
