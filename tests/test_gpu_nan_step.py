"""optimizeSet calls that end with a NaN step (DMSA_STOP_NAN; DmsaOptimizer.h:116-122: setPoseParameters(paramVec); break), which the product
spreads over five solver tails, k_loop_chain's early return, a branch of k_loop_finish of its own and a host that learns of the stop one
synchronisation late (csrc/loop_kernels.hip, csrc/optimize_loop.cpp).  The problems and systems are those of tests/nan_step_cases.py; what the
CPU oracle does with each of them is asserted in tests/test_nan_step_cases.py.  Every comparison is by bits.

A  the solver tails on steps with ONE NaN entry, at 0, P - 1 and on both sides of the 64-boundaries, each followed on the same context by a
   well-posed system whose step must be the oracle's (the panel and stream solves reuse their scratch under a new epoch)
B  whole calls against the oracle -- report, trace, poses, global points -- and every variant of the loop against the default run
C  a context after such a call: ordinary problem, NaN problem, the ordinary one again, another one, each the oracle's run on a fresh state

Which code a case reaches (P: k_loop_lm_step up to 64; k_loop_lm_stream + k_loop_lm_stream_tail up to 192, k_loop_lm_panels with lm_stream = 0
and up to 1024; beyond, the host solve and k_loop_step_finish):
  window_* and keyframes_*_P30, keyframes_odometry_measurement   k_loop_lm_step<1,4>  (P = 30)
  keyframes_last_frame_P72     the stream tail, and the panels under lm_stream = 0;  _P198  the panels;  _P1194  k_loop_step_finish and the
                               host's own test in front of it (host_nan: the loop ends without the device's answer)
  all of them                  k_loop_finish's NaN branch (window: the relative poses only; keyframes: re-chained) and, with num_iter = 3, the
                               host's break at h_results[iter - 1].stop behind an iteration head that was already enqueued -- with next_head an
                               adoption of index 0 (next_head_iterations = 1); with num_iter = 1 the call ends at the loop's end
  device_loop = 0              the host-driven loop's test (optimize_loop.cpp: anyNan)"""
import dataclasses

import numpy as np
import pytest

import nan_step_cases as nc

pytestmark = pytest.mark.gpu


# ---- A: the solve alone ---------------------------------------------------------------------------------------------------------------
def _solve_cases():
    out = []
    for P, streams in nc.SOLVE_TIERS.items():
        cols = nc.solve_columns(P)
        # (one column per case at the largest size: a system of it takes the oracle three seconds)
        groups = [(c,) for c in cols] if P == 594 else [tuple(cols)]
        out += [(P, lm_stream, g) for lm_stream in streams for g in groups]
    return out


def _nan_then_regular(opt, orc, P, H, g, nan_positions, what):
    step, nan = opt.lmSolveDevice(H, g, 0.2)
    assert nan == bool(nan_positions), (P, what, sorted(nan_positions)[:4])
    Hr, gr, step_ref = nc.regular_system(orc, P)
    step, nan = opt.lmSolveDevice(Hr, gr, 0.2)
    assert not nan, (P, what)
    assert np.array_equal(step.view(np.uint64), step_ref.view(np.uint64)), (P, what, np.abs(step - step_ref).max())


@pytest.mark.parametrize("P,lm_stream,cols", _solve_cases(), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_one_nan_entry_of_the_step_is_seen_wherever_it_lies(hip, orc, P, lm_stream, cols):
    """J[:, c] = 0, no damping: the step is NaN at c alone (test_nan_step_cases.py), so a tail that walked only part of the step would
    answer `no NaN` for some c.  The well-posed system behind every NaN solve must come out as if nothing had been there before."""
    opt = hip.DmsaOptimizer(debug={"lm_stream": lm_stream})
    for c in cols:
        H, g, pos = nc.singular_system(orc, P, "zero_column", (c,), 1000 + P)
        assert pos == {c}
        _nan_then_regular(opt, orc, P, H, g, pos, ("zero_column", c))
    opt.close()


@pytest.mark.parametrize("P,lm_stream", nc.ONE_PER_TIER)
def test_equal_columns_and_a_nan_entry_in_every_tier(hip, orc, P, lm_stream):
    opt = hip.DmsaOptimizer(debug={"lm_stream": lm_stream})
    for kind in ("equal_columns", "nan_entry"):
        H, g, pos = nc.singular_system(orc, P, kind, (P // 2,), 2000 + P)
        assert len(pos) == (2 if kind == "equal_columns" else P)
        for rep in range(2):
            _nan_then_regular(opt, orc, P, H, g, pos, (kind, rep))
    opt.close()


# ---- B: whole calls ---------------------------------------------------------------------------------------------------------------------
def _oracle(orc, name, num_iter, fixed_iters=False, analytic=False):
    prob, s = nc.build(name, num_iter)
    s.use_analytic_jacobi = analytic
    p = prob.copy()
    rep, gl, tr = (orc.optimize_window if nc.is_window(name) else orc.optimize_keyframes)(p, s, fixed_iters=fixed_iters, want_global=True)
    return nc.run_record(p, rep, tr, gl)


def _product(hip, name, num_iter, debug=None, fixed_iters=False, analytic=False):
    """-> (record, counters); no device-side wait of the call may have given up: that is what a signal the NaN path forgot looks like"""
    prob, s = nc.build(name, num_iter)
    s.use_analytic_jacobi = analytic
    p = prob.copy()
    opt = hip.DmsaOptimizer(fixed_iters=fixed_iters, debug=debug)
    rep = opt.optimizeSet(p, s)
    rec = nc.run_record(p, rep, opt.trace(), opt.globalPoints())
    counters = opt.debugCounters()
    opt.close()
    assert counters["sync_retries"] == 0, (name, num_iter, debug, counters)
    return rec, counters


def _variants(name):
    v = [{"device_loop": 0}, {"device_sync": 0}, {"dual_stream": 0}, {"one_readback": 0}, {"one_readback": 1}, {"device_loop": 0, "device_sync": 0}]
    if name == "window_imu_measurement":
        v.append({"trial_rows_aside": 0})
    if name == "keyframes_last_frame_P72":
        v += [{"lm_stream": 1}, {"lm_stream": 0}, {"eval_skip": 0}]
    if name == "keyframes_last_frame_P198":
        v += [{"eval_skip": 0}]
    return v


WHOLE_CALLS = [n for n in nc.NAN_CASES if n not in nc.ORACLE_NEEDS_MINUTES]


@pytest.mark.parametrize("name", WHOLE_CALLS)
def test_a_call_that_ends_with_a_nan_step_equals_the_oracle(hip, orc, name):
    P = nc.build(name)[0].numParams
    for num_iter in (1, 3):  # 1: the call ends at the loop's end; 3: the host has enqueued the next iteration's head before it sees the stop
        ref = _oracle(orc, name, num_iter)
        nc.literal_nan_stop(ref, P)
        dev, _ = _product(hip, name, num_iter)
        nc.literal_nan_stop(dev, P)
        nc.same_run(dev, ref)
        fixed, _ = _product(hip, name, num_iter, fixed_iters=True)  # (fixed iterations run through NO_IMPROVEMENT and EPSILON, not through a NaN)
        nc.same_run(fixed, _oracle(orc, name, num_iter, fixed_iters=True))
        nc.same_run(fixed, dev)
        for debug in _variants(name):
            got, _ = _product(hip, name, num_iter, debug=debug)
            nc.same_run(got, dev)
        if nc.is_window(name) and name != "window_imu_measurement":
            heads = {}
            for mode in (0, 2, 3):
                got, c = _product(hip, name, num_iter, debug={"next_head": mode})
                nc.same_run(got, dev)
                assert c["next_head_mismatches"] == 0, (mode, c)
                heads[mode] = c["next_head_iterations"]
            # the head enqueued behind the NaN iteration adopts index 0, the base table as it stands
            assert heads == ({0: 0, 2: 0, 3: 0} if num_iter == 1 else {0: 0, 2: 1, 3: 1}), heads


@pytest.mark.parametrize("name", ["keyframes_last_frame_P30", "keyframes_last_frame_P72"])
def test_the_analytic_jacobian_meets_the_same_zero_columns(hip, orc, name):
    """use_analytic_jacobi: the emptied frame's columns are zero whichever way J is computed, e0 is the same evaluation 0, and the parameters
    are put back, so the call equals the oracle's in everything but the evaluation count.  The oracle, like the reference, has the setting
    and no code behind it -- it counts the 1 + P evaluations of the forward differences -- while the product's analytic path evaluates the
    residuals once per Jacobian (tests/test_gpu_analytic_jacobian.py: evaluations == 10 x iterations) and, on this path, takes the nine
    trials back: 1."""
    for num_iter in (1, 3):
        ref = _oracle(orc, name, num_iter, analytic=True)
        nc.literal_nan_stop(ref, nc.build(name)[0].numParams)
        ref["ints"] = ref["ints"][:2] + (1,) + ref["ints"][3:]
        dev, _ = _product(hip, name, num_iter, analytic=True)
        nc.literal_nan_stop(dev, None, evaluations=1)
        nc.same_run(dev, ref)
        host, _ = _product(hip, name, num_iter, debug={"device_loop": 0}, analytic=True)
        nc.same_run(host, dev)


def test_the_host_solve_behind_the_device_loop_sees_the_nan(hip):
    """P = 1194: the worker pool solves, the host tests the step itself and ends the loop, k_loop_step_finish raises the device's flag for
    k_loop_finish.  Against the host-driven loop and the outcome spelled out, like the 200-frame set of test_gpu_loop.py."""
    name = "keyframes_last_frame_P1194"
    dev, _ = _product(hip, name, 3)
    nc.literal_nan_stop(dev, 1194)
    assert dev["ints"][3] > 1000 and np.isfinite(dev["floats"][0])
    host, _ = _product(hip, name, 3, debug={"device_loop": 0})
    nc.same_run(host, dev)
    one, _ = _product(hip, name, 1)
    nc.same_run(one, dev)


@pytest.mark.parametrize("name", nc.CONTROLS)
def test_one_step_away_from_the_nan_the_call_runs_every_iteration(hip, orc, name):
    ref = _oracle(orc, name, 3)
    assert ref["ints"][:2] == (3, 0)
    dev, _ = _product(hip, name, 3)
    nc.same_run(dev, ref)
    host, _ = _product(hip, name, 3, debug={"device_loop": 0})
    nc.same_run(host, dev)


# ---- C: the context afterwards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,debug", [("window_tail", {"next_head": 2}), ("keyframes_last_frame_P72", None)], ids=["window_next_head", "keyframes_P72"])
def test_a_context_that_stopped_with_a_nan_step_serves_the_next_calls(hip, orc, name, debug):
    """The stand-in for a NaN step in a later iteration: the NaN call starts from the buffers, the lattice hint and the trial tables a real
    call left behind, and leaves flags, owed signals and speculation state to the calls that follow."""
    window = nc.is_window(name)
    ordinary, other = nc.ordinary(name)
    nan_prob, nan_s = nc.build(name, 3)
    s = dataclasses.replace(nan_s, num_iter=2, lambda_diag=1e-5)  # the reference's damping
    calls = [(ordinary, s), (nan_prob, nan_s), (ordinary, s), (other, s)]
    opt = hip.DmsaOptimizer(debug=debug)
    for i, (prob, st) in enumerate(calls):
        p, q = prob.copy(), prob.copy()
        rep = opt.optimizeSet(p, st)
        got = nc.run_record(p, rep, opt.trace(), opt.globalPoints())
        rep_ref, gl, tr = (orc.optimize_window if window else orc.optimize_keyframes)(q, st, want_global=True)
        ref = nc.run_record(q, rep_ref, tr, gl)
        if i == 1:
            nc.literal_nan_stop(got, prob.numParams)
        else:
            assert ref["ints"][0] == 2, (i, ref["ints"])  # (an ordinary call: both iterations ran)
        nc.same_run(got, ref)
    counters = opt.debugCounters()
    opt.close()
    assert counters["sync_retries"] == 0, counters
