"""Debug switch fit_by_level (csrc/voxelize_driver.cpp): each voxel level's size classes, member gather and Gaussian fit follow that level's own
k_leaf_finalize -- level 1 on the second stream, the size classes and the merged order of the correspondence kernels on the third -- instead
of both gathers, one k_size_classes and one fit in series on the main stream.  No kernel changes its arithmetic, so every case runs the
switch on against the switch off on fresh contexts and compares with np.array_equal; where the suite has the oracle for the shape, the
oracle's bits as well.  No case may leave a device-side wait that gave up behind (sync_retries stays 0)."""
import numpy as np
import pytest

from dmsa_lidar_slam_amd import synth
from dmsa_lidar_slam_amd.problems import DmsaOptimSettings

pytestmark = pytest.mark.gpu

H_INCR = float(np.sqrt(np.finfo(np.float32).eps))
WINDOW = dict(scans=3, rings=16, az_steps=128, num_static=2000)
ON, OFF = {"fit_by_level": 2}, {"fit_by_level": 0}  # (2: whatever the size; the default, 1, takes the new order from 200 000 points on)


def _window(**kw):
    return synth.window_problem(seed=1, **dict(WINDOW, **kw))


def _stage(hip, prob, s, debug, rebuild_with=None):
    """Stage calls: the first fit of a context (no fit guess: every fit launch follows the counts) -> info12 as (information matrix, weight),
    member lists, the residuals E of the Jacobian batch, the per-level class counts.  rebuild_with: a second buildGaussians with other
    settings on the same context first sizes its speculative launches with the counts of the first one."""
    opt = hip.DmsaOptimizer(debug=debug)
    opt.upload(prob)
    base = prob.getPoseParameters()
    P = len(base)
    opt.poseTables(base, download=False)
    opt.updateGlobalPoints(0, download=False)
    M, Mm = opt.buildGaussians(s)
    if rebuild_with is not None:
        M, Mm = opt.buildGaussians(rebuild_with)
    seg, memb, info, w = opt.gaussians()
    classes, by_level = opt.levelSizeClasses()
    opt.poseTables(np.concatenate([base[None], base[None] + H_INCR * np.eye(P)]), download=False)
    E = opt.evalResiduals(P + 1)
    assert opt.debugCounters()["sync_retries"] == 0
    opt.close()
    return dict(M=M, Mm=Mm, seg=seg, memb=memb, info=info, w=w, E=E), classes, by_level


def _same_stage(a, b):
    assert (a["M"], a["Mm"]) == (b["M"], b["Mm"])
    for k in ("seg", "memb", "info", "w", "E"):
        assert np.array_equal(a[k], b[k]), k


def _optimize(hip, problems, s, debug, fixed_iters=True):
    """optimizeSet on one context, problem after problem -> per problem (poses, global points, report, trace)."""
    opt = hip.DmsaOptimizer(fixed_iters=fixed_iters, debug=debug)
    out = []
    for prob in problems:
        p = prob.copy()
        r = opt.optimizeSet(p, s)
        rep = (r.iterations, r.stop_reason, r.evaluations, r.num_gaussians, r.num_gaussians_l1, r.num_memberships, r.error0, r.last_step_norm, r.last_line_search_k)
        tr = [(t["M"], t["M1"], t["Mm"], t["best_k"], t["error0"], t["step_norm"]) for t in opt.trace()[: r.iterations]]
        out.append((p.relOrientations.copy(), p.relTranslations.copy(), opt.globalPoints(), rep, tr))
    counters = opt.debugCounters()
    classes, by_level = opt.levelSizeClasses()
    opt.close()
    assert counters["sync_retries"] == 0, counters
    return out, by_level


def _same_runs(a, b):
    assert len(a) == len(b)
    for (oa, ta, ga, ra, tra), (ob, tb, gb, rb, trb) in zip(a, b):
        assert ra == rb and tra == trb
        assert np.array_equal(oa, ob) and np.array_equal(ta, tb) and np.array_equal(ga, gb)


def _same_as_oracle(run, optimize, prob, s):
    """a whole call as the library's default runs it (it may stop early) against the oracle's: report, trace, poses"""
    p_ref = prob.copy()
    r, _, tr = optimize(p_ref, s)
    assert run[3] == (r.iterations, r.stop_reason, r.evaluations, r.num_gaussians, r.num_gaussians_l1, r.num_memberships, r.error0, r.last_step_norm, r.last_line_search_k)
    assert run[4] == [(t["M"], t["M1"], t["Mm"], t["best_k"], t["error0"], t["step_norm"]) for t in tr[: r.iterations]]
    assert np.array_equal(run[0], p_ref.relOrientations) and np.array_equal(run[1], p_ref.relTranslations)


def _oracle_gaussians(orc, prob, s):
    table, _ = orc.window_pose_table(prob)
    g = orc.transform_points(table, prob.localPoints, prob.tformIdPerPoint)
    glob = np.concatenate([g, prob.staticPoints]).astype(np.float32)
    return orc.Gaussians(glob, np.concatenate([prob.ringIds, prob.staticRingIds]), prob.minGridSize, s), glob


@pytest.fixture(scope="module")
def window_off(hip):
    """The switch off, once: the first fit and Jacobian batch through the stage calls, and three fixed iterations."""
    prob, s = _window(), DmsaOptimSettings.sliding_window(num_iter=3)
    stage, _, by_level = _stage(hip, prob, s, OFF)
    assert not by_level
    runs, by_level = _optimize(hip, [prob], s, OFF)
    assert not by_level
    return prob, s, stage, runs


def test_window_three_iterations(hip, orc, window_off):
    """info12 after the first fit and E of the Jacobian batch (no fit guess: every fit launch follows the counts); then three iterations, of
    which the second and third size their fit launches per level from the previous one's class counts.  Against the switch off and the oracle."""
    prob, s, stage_off, runs_off = window_off
    stage, classes, by_level = _stage(hip, prob, s, ON)
    assert by_level
    _same_stage(stage, stage_off)
    ref, glob = _oracle_gaussians(orc, prob, s)
    assert (stage["M"], stage["Mm"]) == (ref.M, ref.Mm)
    assert np.array_equal(stage["seg"], ref.seg_offset) and np.array_equal(stage["memb"], ref.members)
    assert np.array_equal(stage["info"], ref.info) and np.array_equal(stage["w"], ref.weights)
    assert np.array_equal(stage["E"][0], ref.residuals(glob))
    sizes = np.diff(ref.seg_offset)
    for l, sz in enumerate((sizes[: ref.M1], sizes[ref.M1:])):  # the per-level classes are the level's Gaussians, all of them
        assert classes[l, :3].sum() == sz.size and classes[l, 3] == sz.max()
    runs, by_level = _optimize(hip, [prob], s, ON)
    assert by_level
    _same_runs(runs, runs_off)
    assert _optimize(hip, [prob], s, None)[0][0][3] == runs[0][3]  # (and so is the context's default, whichever side it is)
    _same_as_oracle(_optimize(hip, [prob], s, ON, fixed_iters=False)[0][0], orc.optimize_window, prob, s)


def test_fit_guess_too_small(hip, window_off):
    """The speculative launches cover too little, the launch after the counts tops every level up.  Twice: the same context moves on to a window
    of twice the scans (an upload forgets the guess: every launch follows the counts, on buffers the first problem used); and a second
    buildGaussians on a resident problem whose first one accepted a fraction of the sets (min_num_points_per_set 40 against 10), so that its
    counts are a guess several times too small in every class of every level."""
    prob, s, _, _ = window_off
    big = _window(scans=6)
    on, _ = _optimize(hip, [prob, big], s, ON)
    off, _ = _optimize(hip, [prob, big], s, OFF)
    _same_runs(on, off)
    assert on[1][3][3] > 1.5 * on[0][3][3]  # about twice the Gaussians
    few = DmsaOptimSettings.sliding_window(num_iter=3)
    few.min_num_points_per_set = 40
    a, classes, by_level = _stage(hip, big, few, ON, rebuild_with=s)
    b, _, _ = _stage(hip, big, few, OFF, rebuild_with=s)
    assert by_level
    _same_stage(a, b)
    only, _, _ = _stage(hip, big, s, OFF)
    _same_stage(a, only)  # and the guess left nothing behind
    first, _, _ = _stage(hip, big, few, OFF)
    assert 0 < first["M"] < a["M"] // 3


@pytest.mark.parametrize("small_threshold", [8, 32, 256])
def test_small_threshold_boundaries(hip, window_off, small_threshold):
    prob, s, stage_off, runs_off = window_off
    stage, classes, by_level = _stage(hip, prob, s, dict(ON, small_threshold=small_threshold))
    assert by_level
    _same_stage(stage, stage_off)
    sizes = np.diff(stage["seg"])
    m0 = int(classes[0, :3].sum())
    for l, sz in enumerate((sizes[:m0], sizes[m0:])):  # the per-level short class is the level's Gaussians up to the threshold
        assert classes[l, 2] == (sz <= small_threshold).sum() and classes[l, 0] == 0
    runs, _ = _optimize(hip, [prob], s, dict(ON, small_threshold=small_threshold))
    _same_runs(runs, runs_off)


def test_all_three_fit_classes_in_each_level(hip, orc):
    """long_log2 lowered until each level has Gaussians in the fit's long, middle and short class.  The window of the other cases cannot have
    that: its largest Gaussians have 13 (level 0) and 70 (level 1) members and the switch goes down to 2^9.  The same points on a grid ten
    times as coarse (grid_size 1.5) have sets of up to 799 and 2614 members; long_log2 is chosen here from the oracle's set sizes."""
    prob, s = _window(grid_size=1.5), DmsaOptimSettings.sliding_window(num_iter=3)
    ref, _ = _oracle_gaussians(orc, prob, s)
    sizes = np.diff(ref.seg_offset)
    levels = (sizes[: ref.M1], sizes[ref.M1:])
    small_threshold = 32
    long_log2 = int(np.floor(np.log2(min(sz.max() for sz in levels))))
    assert 9 <= long_log2 <= 20  # the range of the switch
    want = [[(sz >= 1 << long_log2).sum(), ((sz > small_threshold) & (sz < 1 << long_log2)).sum(), (sz <= small_threshold).sum(), sz.max()] for sz in levels]
    assert all(c > 0 for row in want for c in row[:3]), want
    debug = {"small_threshold": small_threshold, "long_log2": long_log2}
    a, classes, by_level = _stage(hip, prob, s, dict(ON, **debug))
    b, _, _ = _stage(hip, prob, s, dict(OFF, **debug))
    assert by_level and classes.tolist() == [[int(c) for c in row] for row in want], (classes, want)
    _same_stage(a, b)
    assert np.array_equal(a["info"], ref.info) and np.array_equal(a["w"], ref.weights) and np.array_equal(a["seg"], ref.seg_offset)
    on, _ = _optimize(hip, [prob], s, dict(ON, **debug))
    off, _ = _optimize(hip, [prob], s, dict(OFF, **debug))
    _same_runs(on, off)


@pytest.mark.parametrize("variant", ["level_1_off", "level_0_off", "level_0_accepts_nothing"])
def test_one_level_empty_or_off(hip, orc, variant):
    """A level switched off keeps the common order (nothing to run side by side); a level that is on but accepts no leaf runs by level with an
    empty range -- level 0 of this window has no set of 40 points, level 1 has 39 of them."""
    prob, s = _window(), DmsaOptimSettings.sliding_window(num_iter=3)
    if variant == "level_1_off":
        s.grid_size_2_factor = 0.0
    elif variant == "level_0_off":
        s.grid_size_1_factor = 0.0
    else:
        s.min_num_points_per_set = 40
        s.min_num_gaussians = 5
    a, classes, by_level = _stage(hip, prob, s, ON)
    b, _, _ = _stage(hip, prob, s, OFF)
    _same_stage(a, b)
    assert a["M"] > 0
    if variant == "level_0_accepts_nothing":
        ref, _ = _oracle_gaussians(orc, prob, s)
        assert ref.M1 == 0 and ref.M > 0 and by_level
        assert classes[0].tolist() == [0, 0, 0, 0] and classes[1, :3].sum() == ref.M
        assert np.array_equal(a["info"], ref.info) and np.array_equal(a["w"], ref.weights)
    else:
        assert not by_level
    on, _ = _optimize(hip, [prob], s, ON)
    off, _ = _optimize(hip, [prob], s, OFF)
    _same_runs(on, off)
    assert on[0][3][0] == 3  # three iterations ran


def test_event_dependencies(hip, window_off, monkeypatch):
    """DMSA_DEBUG=device_sync=0: every stream dependency of the new order as a HIP event."""
    prob, s, stage_off, runs_off = window_off
    monkeypatch.setenv("DMSA_DEBUG", "device_sync=0")
    stage, _, by_level = _stage(hip, prob, s, ON)
    assert by_level
    _same_stage(stage, stage_off)
    runs, _ = _optimize(hip, [prob], s, ON)
    _same_runs(runs, runs_off)


def test_keyframes(hip, orc):
    """Keyframe sets go through the same build_gaussians (with splitSet: two slots per leaf): 8 frames, 2 iterations."""
    prob = synth.keyframe_problem(seed=5, frames=8, rings=24, az_steps=160, arc=0.5)
    s = DmsaOptimSettings.keyframe_map(num_iter=2)
    on, by_level = _optimize(hip, [prob], s, ON)
    off, _ = _optimize(hip, [prob], s, OFF)
    assert by_level
    _same_runs(on, off)
    _same_as_oracle(_optimize(hip, [prob], s, ON, fixed_iters=False)[0][0], orc.optimize_keyframes, prob, s)


def test_large_keyframe_set_with_the_host_solver(hip):
    """172 light frames, P = 1026: beyond the panel solve, so the host solves and synchronises in mid-iteration, and the third stream carries the
    1027 chains and pose tables of the Jacobian batch in front of the size classes -- the level fits wait longest here.  An earlier form of the
    order (the classes' wait inside the fit kernel) failed on this shape one run in three: pairs that eval_skip calls equal to evaluation 0 were
    not.  New order forced (the set has 66 000 points, below the default's size rule) against the common one, eval_skip = 2 counting such pairs."""
    prob = synth.keyframe_problem(frames=172, rings=8, az_steps=48, arc=2 * np.pi * 172 / 256.0)
    assert prob.numParams == 1026
    s = DmsaOptimSettings.keyframe_map(num_iter=2)
    out = {}
    for name, sw in (("on", ON), ("off", OFF)):
        opt = hip.DmsaOptimizer(debug=dict(sw, eval_skip=2, skip_stats=1))
        p = prob.copy()
        r = opt.optimizeSet(p, s)
        c = opt.debugCounters()
        _, by_level = opt.levelSizeClasses()
        rep = (r.iterations, r.stop_reason, r.evaluations, r.num_gaussians, r.num_gaussians_l1, r.num_memberships, r.error0, r.last_step_norm, r.last_line_search_k)
        tr = [(t["M"], t["M1"], t["Mm"], t["best_k"], t["error0"], t["step_norm"]) for t in opt.trace()[: r.iterations]]
        opt.close()
        assert by_level == (name == "on")
        assert c["sync_retries"] == 0 and c["skip_mismatches"] == 0 and c["skip_pairs_equal"] > 0, (name, c)
        out[name] = (p.relOrientations, p.relTranslations, rep, tr)
    assert out["on"][2] == out["off"][2] and out["on"][3] == out["off"][3] and out["on"][2][0] == 2
    assert np.array_equal(out["on"][0], out["off"][0]) and np.array_equal(out["on"][1], out["off"][1])
