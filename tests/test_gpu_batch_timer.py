"""Debug switches batch_stamps and one_readback (csrc/optimize_loop.cpp: run_residuals, csrc/voxelize_driver.cpp: enqueue_readback).

batch_stamps: a residual batch whose tiers run on more than one stream is timed by the device's wall clock inside kernels the batch has anyway
(its latency tier stores the begin, the join's wait kernel adds the difference to a tick accumulator) instead of a HIP-event pair on the main
stream; every other batch keeps the pair.  one_readback: lattice tables, counts and the device loop's previous IterResult reach the host in one
copy instead of three.  Neither changes a kernel's arithmetic: every shape runs the four combinations on fresh contexts and compares bits, and
dmsa_timing must make sense whichever way it was measured -- the calls are synchronous, so the batches' time on one stream cannot exceed the
host's wall time around the call."""
import time

import numpy as np
import pytest

from dmsa_lidar_slam_amd import synth
from dmsa_lidar_slam_amd.problems import DmsaOptimSettings

pytestmark = pytest.mark.gpu

COMBOS = ((1, 1), (0, 0), (1, 0), (0, 1))  # (batch_stamps, one_readback)
ITERS = 3
LONG = {"long_log2": 9}  # Gaussians of >= 512 members go to the latency tier: the tiers fork to three streams and join behind a wait kernel


def _config2(use_imu):
    """The points of bench.py's small IMU window (config 2: 25 360 points) on a 0.5 m grid: ten Gaussians of 512 .. 1638 members at the start,
    none of 4096 -- a latency tier with long_log2 = 9, none at the built-in 12."""
    return synth.window_problem(seed=5, scans=5, rings=32, az_steps=96, num_static=10_000, use_imu=use_imu, grid_size=0.5)


SHAPES = {
    "join_wait": (lambda: _config2(False), lambda n: DmsaOptimSettings.sliding_window(num_iter=n), LONG),
    "no_long_gaussian": (lambda: _config2(False), lambda n: DmsaOptimSettings.sliding_window(num_iter=n), {}),
    "imu_window": (lambda: _config2(True), lambda n: DmsaOptimSettings.sliding_window(num_iter=n), dict(LONG, trial_rows_aside=1)),
    # the smallest set tests/test_gpu_large_keyframe_sets.py runs at P = 186 (32 light frames)
    "keyframes_P186": (lambda: synth.keyframe_problem(frames=32, rings=8, az_steps=48, arc=2 * np.pi * 32 / 256.0),
                       lambda n: DmsaOptimSettings.keyframe_map(num_iter=n), LONG),
}


def _switches(combo, extra):
    return dict(extra, batch_stamps=combo[0], one_readback=combo[1])


def _report(r):
    return tuple(getattr(r, name) for name, _ in r._fields_)


def _call(opt, prob, s):
    """one optimizeSet -> (poses, global points, report, trace), the host's wall time around it in ms"""
    p = prob.copy()
    t0 = time.perf_counter()
    r = opt.optimizeSet(p, s)
    wall_ms = 1e3 * (time.perf_counter() - t0)
    tr = [tuple(sorted(t.items())) for t in opt.trace()[: r.iterations]]
    return (p.relOrientations.copy(), p.relTranslations.copy(), opt.globalPoints(), _report(r), tr), wall_ms


def _same(a, b, what):
    assert a[3] == b[3] and a[4] == b[4], what
    for k in range(3):
        assert np.array_equal(a[k], b[k]), (what, k)


def _timing_makes_sense(t, wall_ms, what):
    print(f"[batch timer] {what}: residual_kernel_ms {t.residual_kernel_ms:.4f} in {t.residual_launches} launches, host wall {wall_ms:.3f} ms")
    assert np.isfinite(t.residual_kernel_ms) and 0.0 < t.residual_kernel_ms <= wall_ms, (what, t.residual_kernel_ms, wall_ms)


@pytest.fixture(scope="module")
def runs(hip):
    """shape -> {combo: (result, timing, wall ms)} of one call of three fixed iterations on a fresh context, each computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            make, settings, extra = SHAPES[name]
            prob, s = make(), settings(ITERS)
            out = {}
            for combo in COMBOS:
                opt = hip.DmsaOptimizer(fixed_iters=True, debug=_switches(combo, extra))
                res, wall_ms = _call(opt, prob, s)
                t = opt.timing()
                assert opt.debugCounters()["sync_retries"] == 0
                opt.close()
                out[combo] = (res, t, wall_ms)
            cache[name] = (prob, s, out)
        return cache[name]

    return get


def test_the_join_wait_shape_has_a_latency_tier(hip):
    """The condition of every "join wait" case below: with long_log2 = 9 the library's own first voxelisation of the window has Gaussians
    of the long class, and none at the built-in boundary (2^12 members)."""
    make, settings, _ = SHAPES["join_wait"]
    prob, s = make(), settings(ITERS)
    opt = hip.DmsaOptimizer(debug=dict(LONG, fit_by_level=2))
    opt.upload(prob)
    opt.poseTables(prob.getPoseParameters(), download=False)
    opt.updateGlobalPoints(0, download=False)
    opt.buildGaussians(s)
    sizes = np.diff(opt.gaussians()[0])
    classes, by_level = opt.levelSizeClasses()
    opt.close()
    assert by_level and classes[:, 0].sum() == (sizes >= 512).sum() > 0, (classes, np.sort(sizes)[-5:])
    assert sizes.max() < 4096  # the "no long Gaussian" shape: everything on one stream at the default boundary


@pytest.mark.parametrize("shape", list(SHAPES))
def test_four_switch_combinations_compute_the_same(runs, shape):
    prob, s, out = runs(shape)
    ref = out[COMBOS[0]]
    P = prob.numParams
    for combo in COMBOS:
        res, t, wall_ms = out[combo]
        _same(res, ref[0], (shape, combo))
        assert res[3][0] == ITERS  # report.iterations: all three ran
        assert (t.residual_launches, t.residual_evaluations) == (ref[1].residual_launches, ref[1].residual_evaluations), (shape, combo)
        if shape != "keyframes_P186":
            assert (t.residual_launches, t.residual_evaluations) == (2 * ITERS, (P + 10) * ITERS), (shape, combo)
        _timing_makes_sense(t, wall_ms, (shape, combo))
    assert P == (186 if shape == "keyframes_P186" else 30)


@pytest.mark.parametrize("combo", COMBOS)
def test_reset_and_accumulation(hip, runs, combo):
    prob, s, out = runs("join_wait")
    opt = hip.DmsaOptimizer(fixed_iters=True, debug=_switches(combo, LONG))
    res, wall1 = _call(opt, prob, s)
    _same(res, out[combo][0], combo)
    t1 = opt.timing()
    _timing_makes_sense(t1, wall1, (combo, "first call"))
    res, wall2 = _call(opt, prob, s)
    t2 = opt.timing(reset=True)
    assert t2.residual_launches == 2 * t1.residual_launches and t2.residual_evaluations == 2 * t1.residual_evaluations
    assert t2.residual_kernel_ms > t1.residual_kernel_ms
    _timing_makes_sense(t2, wall1 + wall2, (combo, "two calls"))
    t0 = opt.timing()
    assert (t0.residual_kernel_ms, t0.residual_launches, t0.residual_evaluations, t0.total_ms) == (0.0, 0, 0, 0.0)
    res, wall3 = _call(opt, prob, s)  # and the accumulators start again from there
    t3 = opt.timing()
    assert t3.residual_launches == t1.residual_launches
    _timing_makes_sense(t3, wall3, (combo, "after the reset"))
    opt.close()


@pytest.mark.parametrize("combo", COMBOS)
def test_three_hundred_iterations_in_one_call(hip, combo):
    make, settings, extra = SHAPES["join_wait"]
    prob, s = make(), settings(300)
    opt = hip.DmsaOptimizer(fixed_iters=True, debug=_switches(combo, extra))
    res, wall_ms = _call(opt, prob, s)
    t = opt.timing()
    opt.close()
    assert res[3][0] == 300 and t.residual_launches == 600 and t.residual_evaluations == 300 * (prob.numParams + 10)
    _timing_makes_sense(t, wall_ms, (combo, "300 iterations"))


def test_a_timed_out_wait_reruns_the_call_on_events(hip, runs):
    """sync_fault = 4 withholds the signal of the call's fourth device-side wait: the call runs again with event dependencies, where no batch has
    a join wait -- the timer falls back to the event pair, for the rest of this call and for the next one on the context."""
    prob, s, out = runs("join_wait")
    opt = hip.DmsaOptimizer(fixed_iters=True, debug=dict(LONG, sync_fault=4))
    res, wall1 = _call(opt, prob, s)
    _same(res, out[COMBOS[0]][0], "sync_fault")
    assert opt.debugCounters()["sync_retries"] == 1
    t1 = opt.timing()
    _timing_makes_sense(t1, wall1, "the call that was run again")
    res, wall2 = _call(opt, prob, s)
    _same(res, out[COMBOS[0]][0], "the call after it")
    t2 = opt.timing()
    assert opt.debugCounters()["sync_retries"] == 1 and t2.residual_launches == t1.residual_launches + 2 * ITERS
    assert t2.residual_kernel_ms > t1.residual_kernel_ms
    _timing_makes_sense(t2, wall1 + wall2, "both calls")
    opt.close()


@pytest.mark.parametrize("combo", [(1, 1), (0, 0)])
def test_stage_timers(hip, runs, combo):
    prob, s, out = runs("join_wait")
    opt = hip.DmsaOptimizer(fixed_iters=True, stage_timers=True, debug=_switches(combo, LONG))
    res, wall_ms = _call(opt, prob, s)
    t = opt.timing()
    opt.close()
    _same(res, out[combo][0], combo)
    for name in ("residual_kernel_ms", "voxelize_ms", "gaussian_fit_ms", "pose_table_ms", "normal_eq_ms", "total_ms"):
        assert getattr(t, name) > 0.0, (combo, name)
    _timing_makes_sense(t, wall_ms, (combo, "stage timers"))


def test_a_wrong_sort_width_guess_with_one_readback(hip, runs):
    """speculation_fault = 2: the second voxelisation's guess is too small, seen in the one read-back; the re-run reads the lattice tables without
    speculation (sync #1) through the view into the read-back block."""
    prob, s, out = runs("join_wait")
    general = dict(LONG, small_voxel=0)
    clean = hip.DmsaOptimizer(fixed_iters=True, debug=_switches((1, 1), general))
    want, _ = _call(clean, prob, s)
    assert clean.debugCounters()["speculation_retries"] == 0
    clean.close()
    _same(want, out[(1, 1)][0], "small_voxel = 0")
    opt = hip.DmsaOptimizer(fixed_iters=True, debug=_switches((1, 1), dict(general, speculation_fault=2)))
    res, wall_ms = _call(opt, prob, s)
    c, t = opt.debugCounters(), opt.timing()
    opt.close()
    _same(res, want, "speculation_fault")
    assert c["speculation_retries"] == 1 and c["sync_retries"] == 0, c
    _timing_makes_sense(t, wall_ms, "speculation_fault")
