"""The systems of tests/lm_pivot_cases.py on the CPU: the plain model of the solve (Gauss-Jordan with partial pivoting, first strict maximum
from row k down) is the oracle's solve (orc_lm_solve, the tail of its lm_step) and the host solve of the product (dmsa_lm_solve, serial and
blocked on 3 and 8 threads) bit for bit -- on systems that swap rows at most steps and meet equal |x| in the pivot column, which the
forward-difference systems of the older tests never do.  Every case prints the swaps and ties the model counted, and proves with
tie="last" that a wrong tie-break would show."""
import ctypes as C

import numpy as np
import pytest

import lm_pivot_cases as lp
import nan_step_cases as cases
from dmsa_lidar_slam_amd import _capi as capi

CASES = [(P, name) for P in lp.TIERS for name in lp.case_names(P)]


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def _host_step(lib, H, g, alpha, threads):
    P = g.size
    Hc, gv, step = np.ascontiguousarray(H.T), np.ascontiguousarray(g), np.zeros(P)  # column-major
    assert lib.dmsa_lm_solve(capi.ptr(Hc, C.c_double), capi.ptr(gv, C.c_double), P, float(alpha), threads, capi.ptr(step, C.c_double)) == capi.DMSA_OK
    return step


def _family(name):
    return "planted" if name.startswith("planted_") else name


@pytest.mark.parametrize("P,name", CASES, ids=[f"{P}-{name}" for P, name in CASES])
def test_model_equals_the_oracle_and_the_host_solve(lib, orc, P, name):
    H, g, alpha, step, swaps, ties_diag, ties_off, log = lp.expected(orc, name, P)
    later = sum(1 for k, _ in log if k > 0)
    print(f"[lm_pivots] P={P} {name}: {swaps} swaps in {P} steps, tie steps with the diagonal {ties_diag}, without {ties_off}, at k > 0 {later}")
    assert np.isfinite(step).all()
    assert np.array_equal(lp.bits(orc.lm_solve(H, g, alpha)), lp.bits(step)), "orc_lm_solve"
    for threads in (1, 3, 8):
        assert np.array_equal(lp.bits(_host_step(lib, H, g, alpha, threads)), lp.bits(step)), ("dmsa_lm_solve", threads)
    family = _family(name)
    if family == "scaled_gram":
        e0, J = lp.scaled_gram_jacobian(P)
        assert np.array_equal(lp.bits(orc.lm_step_from_jacobian(e0, J, lp.LAMBDA, alpha)[2]), lp.bits(step)), "orc_lm_step_from_jacobian"
        assert np.array_equal(H, H.T)
    # ---- what the family is for ----
    if family in ("general", "scaled_gram"):
        assert 2 * swaps >= P, (swaps, P)
    if family in ("paired_rows", "planted"):
        last = lp.model_step(H, g, alpha, tie="last")[0]
        changed = int((lp.bits(last) != lp.bits(step)).sum())
        print(f"[lm_pivots] P={P} {name}: taking the LAST tied row changes {changed} of {P} components")
        assert changed > 0
    if family == "paired_rows":
        assert later >= P // 10, (later, P)
    if family == "planted":
        a, b = (int(x) for x in name.split("_")[1:])
        assert log[0] == (0, (a, b)), log[:1]
    if family in ("hadamard", "hadamard8"):
        need_diag, need_off = lp.hadamard_ties_wanted(P)
        assert ties_diag >= need_diag and ties_off >= need_off, (ties_diag, ties_off)
        assert int((H == 0.0).sum()) == P * P - sum(n * n for n in lp.hadamard_blocks(P, lp.SMALL_BLOCK if family == "hadamard8" else None))
        closed = lp.hadamard_closed_form_step(P, lp.SMALL_BLOCK if family == "hadamard8" else None)
        if family == "hadamard8":  # exact: the closed form bit for bit, whatever the tie order
            assert np.array_equal(lp.bits(step), lp.bits(closed))
            assert np.array_equal(lp.bits(lp.model_step(H, g, alpha, tie="last")[0]), lp.bits(step))
        else:
            err = float(np.abs(step - closed).max())
            print(f"[lm_pivots] P={P} hadamard: |step - closed form| = {err:.3e}, bound {lp.hadamard_closed_form_bound(P):.3e}, "
                  f"exact {np.array_equal(lp.bits(step), lp.bits(closed))}")
            assert err <= lp.hadamard_closed_form_bound(P)
            if max(lp.hadamard_blocks(P)) <= lp.SMALL_BLOCK:
                assert np.array_equal(lp.bits(step), lp.bits(closed))


@pytest.mark.parametrize("P", [30, 186])
def test_the_forward_difference_systems_make_no_swap_and_no_tie(orc, P):
    """tests/nan_step_cases.py::regular_system (= tests/test_gpu_loop.py::_system): strongly diagonally dominant, and the duplicated column leaves
    the diagonal larger by lambda -- the pivot search always keeps the diagonal.  The systems above are what exercises it."""
    H, g, step_ref = cases.regular_system(orc, P)
    step, swaps, ties_diag, ties_off = lp.model_step(H, g, 0.2)
    print(f"[lm_pivots] regular_system P={P}: {swaps} swaps, {ties_diag + ties_off} tie steps")
    assert np.array_equal(lp.bits(step), lp.bits(step_ref))
    assert (swaps, ties_diag, ties_off) == (0, 0, 0)
