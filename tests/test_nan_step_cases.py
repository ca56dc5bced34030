"""What the CPU oracle does with the problems and systems of tests/nan_step_cases.py -- the statements tests/test_gpu_nan_step.py relies on when
it holds the product against the oracle: every named case leaves optimizeSet through the NaN test of DmsaOptimizer.h:116-122 in its first
iteration, the two controls (the same inputs one step away from the NaN) do not, and a zero column of J puts a NaN into exactly one entry of
the step, so that a solver tail which tested only part of the step would be seen."""
import numpy as np
import pytest

import nan_step_cases as nc


def _oracle(orc, name, num_iter):
    prob, s = nc.build(name, num_iter)
    p = prob.copy()
    rep, _, tr = (orc.optimize_window if nc.is_window(name) else orc.optimize_keyframes)(p, s)
    return prob, p, nc.run_record(p, rep, tr)


@pytest.mark.parametrize("num_iter", [1, 3])
@pytest.mark.parametrize("name", [n for n in nc.NAN_CASES if n not in nc.ORACLE_NEEDS_MINUTES])
def test_the_oracle_stops_with_a_nan_step_in_the_first_iteration(orc, name, num_iter):
    prob, after, rec = _oracle(orc, name, num_iter)
    nc.literal_nan_stop(rec, prob.numParams)
    assert np.isnan(rec["floats"][0]) == (name in nc.ERROR0_IS_NAN), rec["floats"]
    # setPoseParameters(paramVec) restores the parameters; centralise / decentralise moves a window's poses all the same (3e-4 m), so the
    # poses a run is compared with are the oracle's, not the input's
    assert np.isfinite(after.getPoseParameters()).all()
    assert np.abs(after.getPoseParameters() - prob.getPoseParameters()).max() < 1e-3
    if name == "window_tail":
        assert rec["ints"][3] == 30  # Gaussians: exactly min_num_gaussians -- one more emptied point and the call stops for that instead
    if name == "keyframes_last_frame_P30":
        assert rec["ints"][3] == 584


def test_the_largest_case_is_the_200_frame_set_with_its_last_frame_emptied():
    """P = 1194 takes the oracle minutes: the construction only"""
    name = "keyframes_last_frame_P1194"
    prob, s = nc.build(name)
    whole = nc.keyframes(name)
    a = int(prob.frameOffsets[-2])
    assert prob.numParams == 1194 and s.lambda_diag == 0.0 and prob.localPoints.shape[0] - a > 0
    assert not np.isfinite(prob.localPoints[a:, :3]).any()
    assert np.array_equal(prob.localPoints[:a], whole.localPoints[:a]) and np.array_equal(prob.localPoints[a:, 3], whole.localPoints[a:, 3])
    for k in ("relOrientations", "relTranslations", "frameOffsets", "localNormals", "ringIds"):
        assert np.array_equal(getattr(prob, k), getattr(whole, k)), k


@pytest.mark.parametrize("num_iter", [1, 3])
@pytest.mark.parametrize("name", nc.CONTROLS)
def test_one_step_away_from_the_nan_the_oracle_runs_every_iteration(orc, name, num_iter):
    prob, after, rec = _oracle(orc, name, num_iter)
    assert rec["ints"][:2] == (num_iter, 0), rec["ints"]
    assert rec["ints"][2] == num_iter * (1 + prob.numParams + 9)
    assert all(np.isfinite(t[4]) and t[5] > 0.0 for t in rec["trace"])
    assert not np.isfinite(prob.localPoints[:, :3]).all()  # (a frame of it is empty like in the NaN case)


@pytest.mark.parametrize("name", ["window_tail", "keyframes_last_frame_P72"])
def test_the_ordinary_problems_around_the_nan_call_run_two_iterations(orc, name):
    """the calls in front of and behind the NaN call on one context (the GPU test's part C) are real ones, with the reference's damping"""
    import dataclasses

    s = dataclasses.replace(nc.build(name, 3)[1], num_iter=2, lambda_diag=1e-5)
    for prob in nc.ordinary(name):
        rep, _, tr = (orc.optimize_window if nc.is_window(name) else orc.optimize_keyframes)(prob.copy(), s)
        assert rep.iterations == 2 and rep.num_gaussians >= s.min_num_gaussians and tr[0]["best_k"] > 0, (rep.iterations, rep.stop_reason, tr)


SOLVE_CASES =[(P, c) for P in nc.SOLVE_TIERS for c in nc.solve_columns(P)]


@pytest.mark.parametrize("P,c", SOLVE_CASES)
def test_a_zero_column_puts_one_nan_into_the_step(orc, P, c):
    """Every (P, c) of the GPU test gives a step that is NaN at c and finite everywhere else -- among them 0, P - 1 and both sides of the
    64-boundaries, where one lane's or one wave's share of the step ends."""
    _, _, pos = nc.singular_system(orc, P, "zero_column", (c,), 1000 + P)
    assert pos == {c}, sorted(pos)


def test_the_column_lists_hold_the_edges():
    for P in nc.SOLVE_TIERS:
        cs = set(nc.solve_columns(P))
        assert {0, P - 1} <= cs
        assert all({b - 1, b} <= cs for b in ((64,) if P == 594 else (64, 128)) if b < P), (P, sorted(cs))


@pytest.mark.parametrize("P", sorted({P for P, _ in nc.ONE_PER_TIER}))
def test_equal_columns_give_two_nans_and_a_nan_entry_fills_the_step(orc, P):
    _, _, pos = nc.singular_system(orc, P, "equal_columns", (P // 2,), 2000 + P)
    assert pos == {0, P // 2}
    H, _, pos = nc.singular_system(orc, P, "nan_entry", (P // 2,), 2000 + P)
    assert len(pos) == P and np.isnan(H[P // 2, P // 2]) and np.isfinite(H).sum() == (P - 1) * (P - 1)


def test_same_run_compares_bits():
    """NaN equals NaN, -0.0 does not equal 0.0, and a NaN does not pass for a number"""
    from types import SimpleNamespace as NS

    def rec(error0, point=1.0):
        rep = NS(iterations=1, stop_reason=2, evaluations=31, num_gaussians=5, num_gaussians_l1=5, num_memberships=9, last_line_search_k=0, error0=error0,
                 last_step_norm=0.0)
        prob = NS(relOrientations=np.zeros((2, 3)), relTranslations=np.ones((2, 3)))
        return nc.run_record(prob, rep, [dict(M=5, M1=5, Mm=9, best_k=0, error0=0.0, step_norm=0.0)], np.array([[point, 0, 0, 1]], np.float32))

    nc.same_run(rec(float("nan")), rec(float("nan")))
    nc.same_run(rec(1.5, float("nan")), rec(1.5, float("nan")))
    for a, b in ((rec(0.0), rec(-0.0)), (rec(float("nan")), rec(1.0)), (rec(1.0, float("nan")), rec(1.0, 2.0)), (rec(1.0, 0.0), rec(1.0, -0.0))):
        with pytest.raises(AssertionError):
            nc.same_run(a, b)
    nc.literal_nan_stop(rec(float("nan")), 30)
    with pytest.raises(AssertionError):
        nc.literal_nan_stop(rec(1.0), 31)
