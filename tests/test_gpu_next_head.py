"""Debug switch next_head (csrc/optimize_loop.cpp): from the second iteration of a call on, the device loop of a window without IMU rows does
not compute its base pose table.  k_loop_finish leaves the index of the winning line-search trial on the device (0: none won, the loop stopped,
the step was NaN), and k_transform_aabb_adopt takes that trial's table -- or, for 0, the base table as it stands -- and copies it to where the
fit reads it.  No kernel changes its arithmetic, so every case runs the switch at 2 against 0 on fresh contexts and compares poses, global
points, report and trace with np.array_equal; once per shape it also runs 3, which computes the table the old way as well and counts the words
that differ (next_head_mismatches).  next_head_iterations says how many iterations adopted their table: every one but the first of each call
where the switch engages, none where the rule keeps it off (IMU rows, keyframe sets, stage timers).  No case may leave a device-side wait that
gave up behind (sync_retries stays 0).

A NaN step inside a whole call (DMSA_STOP_NAN), on which k_loop_finish writes index 0 like on a stop and the iteration enqueued behind it
adopts the base table as it stands: tests/test_gpu_nan_step.py, on the problems of tests/nan_step_cases.py.

The shapes and iteration counts were chosen with the CPU oracle: the small window's line search gives best_k = 5 5 2 2 2 1 1 0 0 0 in ten fixed
iterations and stops with NO_IMPROVEMENT in the eighth when early exits are on; its step norms are 0.204 and 0.133 in the first two iterations, so
epsilon = 0.15 stops the second one with EPSILON; the one-block window (964 points, 38 Gaussians) gives 1 2 1 0."""
import numpy as np
import pytest

from dmsa_lidar_slam_amd import synth
from dmsa_lidar_slam_amd.problems import DmsaOptimSettings

pytestmark = pytest.mark.gpu

ON, OFF, CHECK = {"next_head": 2}, {"next_head": 0}, {"next_head": 3}
STOP_NO_IMPROVEMENT, STOP_EPSILON = 3, 4  # include/dmsa_hip.h: dmsa_stop_reason


def _small_window():
    """8 144 points: eight blocks of 1 024, the last one partial"""
    return synth.window_problem(seed=1, scans=3, rings=16, az_steps=128, num_static=2000)


def _one_block():
    """964 points, one partial block, 38 Gaussians on a 1 m grid"""
    return synth.window_problem(seed=5, scans=3, rings=8, az_steps=36, num_static=100, grid_size=1.0)


def _optimize(hip, problems, s, debug, fixed_iters=True, **ctx_args):
    """optimizeSet on one context, problem after problem -> per problem (poses, global points, report, trace), and the context's counters"""
    opt = hip.DmsaOptimizer(fixed_iters=fixed_iters, debug=debug, **ctx_args)
    out = []
    for prob in problems:
        p = prob.copy()
        r = opt.optimizeSet(p, s)
        rep = (r.iterations, r.stop_reason, r.evaluations, r.num_gaussians, r.num_gaussians_l1, r.num_memberships, r.error0, r.last_step_norm, r.last_line_search_k)
        tr = [(t["M"], t["M1"], t["Mm"], t["best_k"], t["error0"], t["step_norm"]) for t in opt.trace()[: r.iterations]]
        out.append((p.relOrientations.copy(), p.relTranslations.copy(), opt.globalPoints(), rep, tr))
    counters = opt.debugCounters()
    opt.close()
    assert counters["sync_retries"] == 0, counters
    return out, counters


def _same_runs(a, b):
    assert len(a) == len(b)
    for (oa, ta, ga, ra, tra), (ob, tb, gb, rb, trb) in zip(a, b):
        assert ra == rb and tra == trb
        assert np.array_equal(oa, ob) and np.array_equal(ta, tb) and np.array_equal(ga, gb)


def _best_ks(run):
    return [t[3] for t in run[4]]


def _on_off_check(hip, problems, s, extra=None, **kw):
    """2 against 0, then 3: same bits, no mismatching word; -> the runs with the switch off, the counters with it on"""
    extra = extra or {}
    off, c_off = _optimize(hip, problems, s, dict(OFF, **extra), **kw)
    on, c_on = _optimize(hip, problems, s, dict(ON, **extra), **kw)
    chk, c_chk = _optimize(hip, problems, s, dict(CHECK, **extra), **kw)
    _same_runs(on, off)
    _same_runs(chk, off)
    assert c_off["next_head_iterations"] == 0 and c_off["next_head_mismatches"] == 0, c_off
    assert c_on["next_head_mismatches"] == 0 and c_chk["next_head_mismatches"] == 0, (c_on, c_chk)
    assert c_chk["next_head_iterations"] == c_on["next_head_iterations"]
    return off, c_on


@pytest.fixture(scope="module")
def small_fixed(hip):
    """ten fixed iterations of the small window with the switch off, 2 and 3"""
    prob, s = _small_window(), DmsaOptimSettings.sliding_window(num_iter=10)
    off, c_on = _on_off_check(hip, [prob], s)
    return prob, s, off, c_on


def test_small_window_every_outcome(hip, small_fixed):
    """The trace of the switch-off run has a best_k = 0 that another iteration follows (the base table stays) and three different winning
    trials (three different slots adopted)."""
    prob, s, off, c_on = small_fixed
    ks = _best_ks(off[0])
    assert len(ks) == 10
    assert any(k == 0 for k in ks[:-1]), ks
    assert len({k for k in ks[:-1] if k > 0}) >= 3, ks
    assert c_on["next_head_iterations"] == 9
    default, c_default = _optimize(hip, [prob], s, None)  # the context's default takes the new order at this size as well
    _same_runs(default, off)
    assert c_default["next_head_iterations"] == 9


def test_one_block(hip):
    prob, s = _one_block(), DmsaOptimSettings.sliding_window(num_iter=4)
    assert prob.localPoints.shape[0] + prob.staticPoints.shape[0] < 1024
    off, c_on = _on_off_check(hip, [prob], s)
    ks = _best_ks(off[0])
    assert len(ks) == 4 and any(k > 0 for k in ks[:-1]) and off[0][3][3] >= s.min_num_gaussians, (ks, off[0][3])
    assert c_on["next_head_iterations"] == 3


def test_calls_of_other_sizes_on_one_context(hip):
    """One block, then eight (the trial tables and the check table grow, the lattice hint is stale), then one block again on buffers that
    hold the larger window's tables."""
    small, big, s = _one_block(), _small_window(), DmsaOptimSettings.sliding_window(num_iter=4)
    off, c_on = _on_off_check(hip, [small, big, small], s)
    assert [r[3][0] for r in off] == [4, 4, 4]
    assert c_on["next_head_iterations"] == 9
    _same_runs(off[2:], off[:1])  # (a call leaves nothing behind that the next one reads)


def test_forced_replay(hip, small_fixed):
    """lattice_hint = 0: every voxelisation replays the lattice"""
    prob, s, off_hint, _ = small_fixed
    off, c_on = _on_off_check(hip, [prob], s, extra={"lattice_hint": 0})
    _same_runs(off, off_hint)
    assert c_on["next_head_iterations"] == 9 and c_on["lattice_hints_held"] == 0


def test_event_dependencies(hip, small_fixed, monkeypatch):
    """DMSA_DEBUG=device_sync=0: the side stream's chains follow a HIP event recorded behind the adopting kernel"""
    prob, s, off, _ = small_fixed
    monkeypatch.setenv("DMSA_DEBUG", "device_sync=0")
    on, c = _optimize(hip, [prob], s, ON)
    _same_runs(on, off)
    assert c["next_head_iterations"] == 9


@pytest.mark.parametrize("stop", [STOP_NO_IMPROVEMENT, STOP_EPSILON])
def test_early_exits(hip, orc, stop):
    """A stopped loop: k_loop_finish leaves index 0, and the iteration already enqueued behind it reads no trial table."""
    prob, s = _small_window(), DmsaOptimSettings.sliding_window(num_iter=10)
    if stop == STOP_EPSILON:
        s.epsilon = 0.15
    off, c_on = _on_off_check(hip, [prob], s, fixed_iters=False)
    rep = off[0][3]
    assert rep[1] == stop and rep[0] == (8 if stop == STOP_NO_IMPROVEMENT else 2), rep
    assert c_on["next_head_iterations"] == rep[0]  # iterations 2 .. rep[0], and the one enqueued behind the stop
    p_ref = prob.copy()
    r, _, tr = orc.optimize_window(p_ref, s)
    assert rep == (r.iterations, r.stop_reason, r.evaluations, r.num_gaussians, r.num_gaussians_l1, r.num_memberships, r.error0, r.last_step_norm, r.last_line_search_k)
    assert np.array_equal(off[0][0], p_ref.relOrientations) and np.array_equal(off[0][1], p_ref.relTranslations)


def test_imu_window_keeps_the_present_order(hip):
    """The small IMU window of bench.py at its real size (25 360 points).  Off by rule: updateImuError rewrites relative pose 0 in every
    evaluation, so the next iteration's chain does not start from the pose 0 trial k ran on.  2 changes nothing and adopts nothing."""
    prob = synth.window_problem(seed=5, scans=5, rings=32, az_steps=96, num_static=10_000, use_imu=True)
    assert prob.localPoints.shape[0] + prob.staticPoints.shape[0] == 25_360
    s = DmsaOptimSettings.sliding_window(use_imu=True, num_iter=4)
    off, c_off = _optimize(hip, [prob], s, OFF)
    on, c_on = _optimize(hip, [prob], s, ON)
    _same_runs(on, off)
    assert off[0][3][0] == 4 and c_on["next_head_iterations"] == 0 and c_off["next_head_iterations"] == 0


def test_keyframe_neighbourhood_keeps_the_present_order(hip):
    prob = synth.keyframe_problem(seed=5, frames=8, rings=24, az_steps=160, arc=0.5)
    s = DmsaOptimSettings.keyframe_map(num_iter=2)
    off, _ = _optimize(hip, [prob], s, OFF)
    for sw in (ON, CHECK):
        on, c = _optimize(hip, [prob], s, sw)
        _same_runs(on, off)
        assert on[0][3][0] == 2 and c["next_head_iterations"] == 0 and c["next_head_mismatches"] == 0


def test_stage_timers_keep_the_present_order(hip, small_fixed):
    """pose_table_ms of a context with stage timers is k_window_pose_tables' time: such a context computes every base table"""
    prob, s, off, _ = small_fixed
    on, c = _optimize(hip, [prob], s, ON, stage_timers=True)
    _same_runs(on, off)
    assert c["next_head_iterations"] == 0
