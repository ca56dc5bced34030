"""The three device LM solves (csrc/loop_kernels.hip: k_loop_lm_step up to 64 parameters, k_loop_lm_stream up to 192, k_loop_lm_panels beyond
and with lm_stream = 0) on the systems of tests/lm_pivot_cases.py: row swaps at most steps, equal |x| in the pivot column at step 0 and after
earlier swaps, between neighbouring waves and between two register slots of one lane -- every step the bits of the plain model, which
tests/test_lm_pivot_cases.py pins to the oracle and to the host solve.  Each solve has its own pivot search, its own tie rule and its own
logical-to-physical row bookkeeping; the forward-difference systems of tests/test_gpu_loop.py make no swap and no tie."""
import numpy as np
import pytest

import lm_pivot_cases as lp

pytestmark = pytest.mark.gpu

FAMILIES = ("general", "scaled_gram", "paired_rows", "planted", "hadamard", "hadamard8")
CASES = [(P, lm_stream, family) for P, streams in lp.TIERS.items() for lm_stream in streams for family in FAMILIES
         if P != lp.LARGEST or family in ("general", "paired_rows")]


@pytest.fixture(scope="module")
def contexts(hip):
    """one context per value of lm_stream, kept for the whole module: every solve reuses the scratch of the ones before it"""
    opts = {1: hip.DmsaOptimizer(debug={"lm_stream": 1}), 0: hip.DmsaOptimizer(debug={"lm_stream": 0})}
    yield opts
    for opt in opts.values():
        opt.close()


def _names(P, family):
    return [n for n in lp.case_names(P) if n == family or (family == "planted" and n.startswith("planted_"))]


def _check(opt, orc, name, P, what):
    H, g, alpha, step_ref, swaps, ties_diag, ties_off, _ = lp.expected(orc, name, P)
    for rep in range(2):  # the panel solve reuses its scratch with a new epoch
        step, nan = opt.lmSolveDevice(H, g, alpha)
        assert not nan, (what, name, rep)
        differing = int((lp.bits(step) != lp.bits(step_ref)).sum())
        assert differing == 0, (what, name, rep, f"{differing} of {P} components differ, max {np.abs(step - step_ref).max():.3e}; the model made {swaps} swaps, "
                                                 f"{ties_diag} + {ties_off} tie steps")
    max_step = 0.37 * np.abs(step_ref).max()  # the clamp of :125-128
    max_elem = max(step_ref.max(), -step_ref.min())
    step, nan = opt.lmSolveDevice(H, g, alpha, max_step)
    assert not nan and np.array_equal(lp.bits(step), lp.bits((max_step / max_elem) * step_ref)), (what, name, "clamped")
    return step_ref


@pytest.mark.parametrize("P,lm_stream,family", CASES, ids=[f"{P}-stream{s}-{f}" for P, s, f in CASES])
def test_device_solve_equals_the_model(contexts, orc, P, lm_stream, family):
    names = _names(P, family)
    assert names
    for name in names:
        step_ref = _check(contexts[lm_stream], orc, name, P, (P, lm_stream))
        if family == "hadamard8":  # exact arithmetic: the closed form H^-1 = H^T / n per block, bit for bit
            assert np.array_equal(lp.bits(step_ref), lp.bits(lp.hadamard_closed_form_step(P, lp.SMALL_BLOCK)))
        if family == "hadamard":   # rounds from order 16 on (lm_pivot_cases.py): the closed form to its bound, the model's bits above
            step, _ = contexts[lm_stream].lmSolveDevice(*lp.system(orc, name, P))
            assert np.abs(step - lp.hadamard_closed_form_step(P)).max() <= lp.hadamard_closed_form_bound(P)


def test_one_context_through_sizes_families_and_both_solves(hip, orc):
    """186 -> 30 -> 200 -> 129 -> 186 on ONE context per lm_stream value, alternating families: the scratch, the epochs and the row
    bookkeeping of a solve are left behind by another size and another permutation -- each result is a fresh context's."""
    route = [(186, "paired_rows"), (30, "general"), (200, "hadamard"), (129, "planted_63_64"), (186, "scaled_gram")]
    for lm_stream in (1, 0):
        used = hip.DmsaOptimizer(debug={"lm_stream": lm_stream})
        for P, name in route:
            H, g, alpha = lp.system(orc, name, P)
            got, nan = used.lmSolveDevice(H, g, alpha)
            fresh_ctx = hip.DmsaOptimizer(debug={"lm_stream": lm_stream})
            fresh, nan_fresh = fresh_ctx.lmSolveDevice(H, g, alpha)
            fresh_ctx.close()
            assert not nan and not nan_fresh
            assert np.array_equal(lp.bits(got), lp.bits(fresh)), (lm_stream, P, name, "used context against a fresh one")
            assert np.array_equal(lp.bits(got), lp.bits(lp.expected(orc, name, P)[3])), (lm_stream, P, name, "against the model")
        used.close()
