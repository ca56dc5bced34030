"""tests/ne_wide_cases.py on the CPU: the oracle's export of blocked_dot (orc_blocked_gram, orc_blocked_squares) is the exact fused chain
above 64 parameters and the numpy restatement of the unfused order up to 64; and the inputs of tests/test_gpu_ne_wide.py can tell the two
rules apart -- a kernel that took the other rule, the other block size or another block order would not pass there."""
import math
from fractions import Fraction

import numpy as np
import pytest

import ne_wide_cases as nw


def test_the_integer_chain_is_the_fraction_formula():
    """fused_chain works on integers for speed; step by step it is float(Fraction(a) * Fraction(b) + Fraction(s))"""
    rng = np.random.default_rng(5)
    scales = (1.0, 1e-160, 1e-300, 5e-324, 1e150, 1e300, 2.0 ** -27)
    for _ in range(4000):
        a, b, s = (float(rng.standard_normal() * rng.choice(scales)) for _ in range(3))
        if rng.integers(4) == 0:
            s = -a * b if math.isfinite(a * b) else 0.0  # the rounded product against the exact one: heavy cancellation
        s = s + 0.0  # (no -0.0: the chain's first step below, fma(1, s, 0), would not hand it on)
        exact = Fraction(a) * Fraction(b) + Fraction(s)
        try:
            want = float(exact)
        except OverflowError:
            want = math.inf if exact > 0 else -math.inf
        got = nw.fused_chain(np.array([1.0, a]), np.array([s, b]))  # fma(1, s, 0) = s, then fma(a, b, s)
        assert nw.bits(got) == nw.bits(want) or (exact == 0 and got == 0.0), (a, b, s, got, want)
        assert nw.bits(got) == nw.bits(nw.fma_exact(a, b, s))
    # what is handled apart
    inf, nan = math.inf, math.nan
    assert nw.fma_exact(inf, 2.0, 1.0) == inf and math.isnan(nw.fma_exact(inf, 0.0, 1.0)) and math.isnan(nw.fma_exact(1.0, nan, 1.0))
    assert nw.fma_exact(1e300, 1e300, -inf) == -inf and nw.fma_exact(1e300, 1e300, 0.0) == inf and nw.fma_exact(-1e300, 1e300, 0.0) == -inf
    assert nw.bits(nw.fma_exact(-0.0, 1.0, 0.0)) == nw.bits(0.0) and nw.bits(nw.fma_exact(-1e-200, 1e-200, 0.0)) == nw.bits(-0.0)
    assert nw.fma_exact(1.0 + 2.0 ** -27, 1.0 + 2.0 ** -27, -1.0) == 2.0 ** -26 + 2.0 ** -54  # one rounding: the low bits of the square survive


def test_the_block_size_rule():
    assert [nw.reduction_block_rows(r, 65) for r in nw.NE_ROWS_LONG] == [256, 256, 256, 256, 288, 288, 320]
    assert [-(-r // nw.reduction_block_rows(r, 65)) for r in nw.NE_ROWS_LONG] == [15, 16, 17, 32, 29, 32, 29]
    assert [nw.reduction_block_rows(r, 65) for r in nw.SQ_ROWS_LONG] == [1024, 1056, 2080]  # one, two and three 1024-row chunks
    assert {nw.reduction_block_rows(r, 64) for r in nw.NE_ROWS_LONG + nw.SQ_ROWS_LONG} == {256}


SAMPLED = [(P, rows) for P in (65, 96, 200) for rows in nw.NE_ROWS] + [(128, 257), (65, 8193), (65, 9217)]


@pytest.mark.parametrize("P,rows", SAMPLED)
def test_oracle_export_equals_the_exact_chain_on_the_sample(orc, P, rows):
    A = nw.columns(nw.batch(P, rows), nw.H_STEP, False)
    Hp = orc.blocked_gram(A, P)
    assert np.array_equal(nw.bits(Hp), nw.bits(Hp.T))
    nw.check_sample(Hp, nw.fused_sample(A, P), (P, rows))


@pytest.mark.parametrize("name", sorted(nw.SPECIAL))
@pytest.mark.parametrize("where", ["e0", "column"])
def test_oracle_export_on_special_values(orc, name, where):
    P, rows = nw.SPECIAL_SHAPES[0]
    for formed in (False, True):
        A = nw.columns(nw.special_batch(P, rows, name, where), 0.5, formed)
        Hp = orc.blocked_gram(A, P)
        nw.check_sample(Hp, nw.fused_sample(A, P), (name, where, formed))
        if name in ("nan", "inf"):
            assert np.isnan(Hp).any() or np.isinf(Hp).any()
        if name == "tiny" and (formed or where == "e0"):  # denormal products, and sums that stay denormal
            c = P if where == "e0" else P - 31
            assert 0.0 < Hp[c, c] < 2.3e-308, Hp[c, c]


@pytest.mark.parametrize("P,rows", nw.NE_CASES)
def test_the_random_cases_tell_the_fused_rule_from_the_unfused(orc, P, rows):
    A = nw.columns(nw.batch(P, rows), nw.H_STEP, False)
    fused, unfused = orc.blocked_gram(A, P), nw.unfused_gram(A, nw.reduction_block_rows(rows, P))
    differing = int((nw.bits(fused) != nw.bits(unfused)).sum())
    print(f"[ne_wide] P={P} rows={rows}: {differing} of {(P + 1) ** 2} elements differ between the fused and the unfused rule")
    if rows == 1:  # one product, rounded once either way: fma(a, b, 0) = a * b
        assert differing == 0
    else:
        assert differing > 0
    if P > 64 and nw.reduction_block_rows(rows, P) != 256:  # the block size shows as well
        assert not np.array_equal(nw.bits(fused), nw.bits(orc.blocked_gram(A, 64)))


def test_up_to_64_parameters_the_export_is_the_unfused_order(orc):
    A = nw.columns(nw.batch(64, 513), nw.H_STEP, False)
    assert np.array_equal(nw.bits(orc.blocked_gram(A, 64)), nw.bits(nw.unfused_gram(A, 256)))


@pytest.mark.parametrize("B,P,rows", nw.SQ_CASES)
def test_squared_sums_of_the_oracle_and_the_models(orc, B, P, rows):
    for kind in ("random", "cancellation"):
        E = nw.squares_input(B, rows, kind)
        rs = nw.reduction_block_rows(rows, P)
        unfused = nw.unfused_squares(E, rs)
        got = orc.blocked_squares(E, P)
        if P <= 64:
            assert np.array_equal(nw.bits(got), nw.bits(unfused)), kind
        else:
            fused = nw.fused_squares(E, P)
            assert np.array_equal(nw.bits(got), nw.bits(fused)), kind
            if kind == "cancellation":
                differing = int((nw.bits(fused) != nw.bits(unfused)).sum())
                print(f"[ne_wide] squared sums B={B} rows={rows}: {differing} of {B} cancellation sums differ between the rules")
                assert differing > 0 or rows == 1  # (one square, rounded once either way)
