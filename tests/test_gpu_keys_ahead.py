"""Debug switch keys_ahead (csrc/voxelize_driver.cpp): a speculated voxelisation makes its leaf codes from the lattice tables the PREVIOUS
voxelisation of the context ended with, beside k_lattice instead of behind it, and the host compares the two sets of tables at its one wait.

Every comparison here is against the same sequence of calls in a context with keys_ahead = 0, bit for bit: everything voxelLevel returns for
both levels, the member lists and the Gaussians; the voxelisation cases also against the oracle and the pointer tree on the global points
the context reports, as tests/test_gpu_lattice_hint.py does.  The counters say which order a build took: keys_ahead_held moves by one per
level of a build whose tables stood, keys_ahead_redone (and speculation_retries) by one per build that was keyed ahead and redone.

The clouds are those of tests/lattice_cases.py (14 373 points: fourteen blocks of 1 024 and a partial one; the `leading_nan` variant starts
with 1 029 non-finite points).  A build follows an upload only once per context: later builds find the depths of the previous one and are
speculated, which is what the ahead order needs.  The points are moved WITHOUT an upload, through the pose tables: two points have a table row
of their own, whose translation setPoseTables changes.

  mover FREE   a core point of the last free block (every event is behind it: it is keyed with the final box of both levels)
  mover TRIG   the trigger at 2 * block + 50, which both levels meet below their box on x

  level 0 only      FREE to x = 800: outside level 0's final box (x < 772.3), inside level 1's (x < 964.75) -- one more event at level 0
  level 1 only      TRIG from x = -1.62 to about -1.0: still below level 0's box of that epoch (x >= -0.5), now inside level 1's (x >= -1.25),
                    whose event at this point disappears; level 0 re-grows the same boxes
  compression only  FREE to x = -500: inside the final boxes of both levels, so both histories stay, but the smallest x of the cloud moves from
                    -1.62 across key 4096 of level 0 (x = -456.5): nbits of that axis 12 -> 13, key_base 1 -> 0

Each of these is checked against the model of the sequential box (lattice_cases.box_history) on the points the context reports, before the
device's verdict is looked at.
"""
import numpy as np
import pytest

import lattice_cases as lc
from dmsa_lidar_slam_amd import synth
from dmsa_lidar_slam_amd.problems import DmsaOptimSettings
from pcl_octree_model import pcl_leaves

pytestmark = pytest.mark.gpu

BLOCK = lc.constants()["kAabbBlock"]
S = DmsaOptimSettings.sliding_window()
AHEAD, PLAIN = {"keys_ahead": 2}, {"keys_ahead": 0}
ROW_FREE, ROW_TRIG = 2, 3
COUNTERS = ("keys_ahead_held", "keys_ahead_redone", "speculation_retries", "lattice_hints_held", "lattice_replays", "small_voxel_fallbacks")


def _tables(dx_free=0.0, dx_trig=0.0):
    t = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (lc.TABLE_ROWS, 1))
    t[ROW_FREE, 3], t[ROW_TRIG, 3] = dx_free, dx_trig
    return t


@pytest.fixture(scope="module")
def plain():
    """the plain cloud, its problem with the two movers on rows of their own, and their indices"""
    base = lc.base_cloud("plain")
    free, trig = base.free_blocks(BLOCK)[-1] * BLOCK + 5, 2 * BLOCK + 50
    assert trig in base.outliers and base.hist(0).epoch[free] == base.hist(0).num_events and base.hist(1).epoch[free] == base.hist(1).num_events
    prob = lc.problem(base)
    assert not (prob.tformIdPerPoint >= 2).any()  # no lone infinity in this cloud: the rows behind the two identities are free
    prob.tformIdPerPoint[free], prob.tformIdPerPoint[trig] = ROW_FREE, ROW_TRIG
    return base, prob, free, trig


def _levels(opt):
    out = []
    for level in (0, 1):
        info, code, key, order = opt.voxelLevel(level)
        out.append(((info.resolution, info.depth, info.num_events, tuple(info.min_xyz), info.num_valid, info.num_leaves), code, key, order))
    return out


def _state(opt, counts):
    return counts, _levels(opt), opt.gaussians()


def _same_state(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    for level in (0, 1):
        assert a[1][level][0] == b[1][level][0], (what, level, a[1][level][0], b[1][level][0])
        for k, name in ((1, "code"), (2, "key"), (3, "order")):
            assert np.array_equal(a[1][level][k], b[1][level][k]), (what, level, name)
    for x, y, name in zip(a[2], b[2], ("seg", "members", "info", "weights")):
        assert x.tobytes() == y.tobytes(), (what, name)


def _against_oracle(orc, state, glob, prob, res_pair, what):
    counts, levels, gauss = state
    for lv, res in enumerate(res_pair):
        info, code, key, order = orc.voxelize(glob, res)
        assert levels[lv][0] == (res, info.depth, info.num_events, tuple(info.min_xyz), info.num_valid, info.num_leaves), (what, lv)
        for got, want, name in zip(levels[lv][1:], (code, key, order), ("code", "key", "order")):
            assert np.array_equal(got, want), (what, lv, name)
        tree, leaves = pcl_leaves(glob, res)
        assert np.array_equal(levels[lv][3], np.concatenate([np.asarray(m, np.int32) for m in leaves])), (what, lv)
        assert (tree.depth, tree.events, tree.mn) == (levels[lv][0][1], levels[lv][0][2], list(levels[lv][0][3])), (what, lv)
    ref = orc.Gaussians(glob, prob.ringIds, prob.minGridSize, S)
    assert counts == (ref.M, ref.Mm), what
    for a, b, name in zip(gauss, (ref.seg_offset, ref.members, ref.info, ref.weights), ("seg", "members", "info", "weights")):
        assert np.array_equal(a, b), (what, name)


def _step(before, after):
    return {k: after[k] - before[k] for k in COUNTERS}


class _Pair:
    """the same calls on a context with keys_ahead = 2 and on one with keys_ahead = 0"""

    def __init__(self, hip, prob, extra=None):
        extra = extra or {}
        self.on, self.off = hip.DmsaOptimizer(debug=dict(AHEAD, **extra)), hip.DmsaOptimizer(debug=dict(PLAIN, **extra))
        self.on.upload(prob), self.off.upload(prob)
        self.glob = None

    def move(self, tables):
        self.on.setPoseTables(tables), self.off.setPoseTables(tables)
        self.glob = self.on.updateGlobalPoints(0)
        assert self.off.updateGlobalPoints(0).tobytes() == self.glob.tobytes()
        return self.glob

    def build(self, what):
        """buildGaussians on both; same bits; -> (state, what the counters of the keys_ahead context moved by)"""
        c0, d0 = self.on.debugCounters(), self.off.debugCounters()
        on, off = _state(self.on, self.on.buildGaussians(S)), _state(self.off, self.off.buildGaussians(S))
        _same_state(on, off, what)
        step, step_off = _step(c0, self.on.debugCounters()), _step(d0, self.off.debugCounters())
        print(f"{what}: keys_ahead=2 {step}; keys_ahead=0 {step_off}")
        assert step_off["keys_ahead_held"] == 0 and step_off["keys_ahead_redone"] == 0, (what, step_off)
        assert step["small_voxel_fallbacks"] == 0 and step["lattice_hints_held"] + step["lattice_replays"] >= 2, (what, step)
        return on, step

    def close(self):
        self.on.close(), self.off.close()


HELD = dict(keys_ahead_held=2, keys_ahead_redone=0, speculation_retries=0)
COMMON = dict(keys_ahead_held=0, keys_ahead_redone=0, speculation_retries=0)
REDONE = dict(keys_ahead_held=0, keys_ahead_redone=1, speculation_retries=1)


def _moved(step, want, what):
    assert {k: step[k] for k in want} == want, (what, step)


@pytest.mark.parametrize("variant", ["plain", "leading_nan"])
def test_second_and_third_build_are_keyed_ahead_and_stand(hip, orc, variant):
    """No upload and no move between the builds: the first one follows the upload (common order, neither counter moves), the next two are
    speculated, keyed from the tables of the one before, and stand.  14 373 points (no multiple of 1 024); `leading_nan`: 1 029 non-finite points."""
    cloud = lc.base_cloud(variant)
    assert cloud.xyz.shape[0] % 1024 != 0 and (variant == "plain" or not np.isfinite(cloud.xyz).all())
    prob = lc.problem(cloud)
    pair = _Pair(hip, prob)
    glob = pair.move(lc.pose_tables())
    first, step = pair.build("first")
    _moved(step, COMMON, "first")
    _against_oracle(orc, first, glob, prob, cloud.res, "first")
    for what in ("second", "third"):
        state, step = pair.build(what)
        _moved(step, HELD, what)
        assert step["lattice_hints_held"] == 2  # the hint, read from the keying set, held too
        _same_state(state, first, what)
    pair.close()


def _history_case(hip, orc, plain, tables, changed_levels, what):
    """first build, a build keyed ahead that stands, the move, a build keyed ahead and redone (the oracle's result for the moved points), the build
    behind the redo in the common order, and a build keyed ahead again"""
    base, prob, _, _ = plain
    pair = _Pair(hip, prob)
    glob0 = pair.move(_tables())
    assert np.array_equal(glob0[:, :3].view(np.uint32), base.xyz.view(np.uint32))
    _moved(pair.build("first")[1], COMMON, what)
    _moved(pair.build("second")[1], HELD, what)
    glob = pair.move(tables)
    for lv in (0, 1):  # the model's verdict on the move, before the device's
        same = lc.box_history(glob[:, :3], base.res[lv]).same_as(base.hist(lv))
        assert same == (lv not in changed_levels), (what, lv, same)
    state, step = pair.build("moved")
    _moved(step, REDONE, what)
    _against_oracle(orc, state, glob, prob, base.res, what)
    again, step = pair.build("behind the redo")
    _moved(step, COMMON, what)
    _same_state(again, state, what)
    again, step = pair.build("ahead again")
    _moved(step, HELD, what)
    _same_state(again, state, what)
    pair.close()
    return glob


def test_a_new_event_at_level_0_only_is_redone(hip, orc, plain):
    base, _, free, _ = plain
    x = 800.0
    assert base.hist(0).mx[-1][0] < x < base.hist(1).mx[-1][0]
    _history_case(hip, orc, plain, _tables(dx_free=x - float(base.xyz[free, 0])), (0,), "level 0 only")


def test_an_event_that_disappears_at_level_1_only_is_redone(hip, orc, plain):
    base, _, _, trig = plain
    e0, e1 = base.hist(0).epoch[trig - 1], base.hist(1).epoch[trig - 1]
    x = -1.0
    assert base.hist(1).mn[e1][0] < x < base.hist(0).mn[e0][0] and float(base.xyz[trig, 0]) < base.hist(1).mn[e1][0]
    _history_case(hip, orc, plain, _tables(dx_trig=x - float(base.xyz[trig, 0])), (1,), "level 1 only")


def _key_ranges(glob, hist):
    """(nbits, key_base) per axis as k_lattice derives them from the bounds of the finite points and the final box"""
    p = glob[np.isfinite(glob[:, :3]).all(axis=1), :3].astype(np.float64)
    depth, out = int(hist.depth[-1]), []
    for a in range(3):
        klo = max(int(np.floor((p[:, a].min() - hist.mn[-1][a]) / hist.res)) - 1, 0)
        khi = min(int(np.floor((p[:, a].max() - hist.mn[-1][a]) / hist.res)) + 1, (1 << depth) - 1)
        bits = 0
        while bits < depth and (klo >> bits) != (khi >> bits):
            bits += 1
        out.append((bits, klo >> bits))
    return out


def test_only_the_compression_changes_and_is_redone(hip, orc, plain):
    base, _, free, _ = plain
    glob = _history_case(hip, orc, plain, _tables(dx_free=-500.0 - float(base.xyz[free, 0])), (), "compression only")
    before = [_key_ranges(np.c_[base.xyz, np.zeros(len(base.xyz))], base.hist(lv)) for lv in (0, 1)]
    after = [_key_ranges(glob, base.hist(lv)) for lv in (0, 1)]
    print("key ranges (nbits, key_base) per axis, level 0 / level 1:", before, "->", after)
    assert before != after


@pytest.mark.parametrize("merge_sort", [0, 1])
def test_both_sort_layouts(hip, orc, plain, merge_sort):
    """merge_sort = 0: a sort per level on two streams; 1: one sort of both levels on the main stream, whose header the first key kernel clears"""
    base, prob, _, _ = plain
    pair = _Pair(hip, prob, extra={"merge_sort": merge_sort})
    glob = pair.move(_tables())
    first, step = pair.build("first")
    _moved(step, COMMON, merge_sort)
    _against_oracle(orc, first, glob, prob, base.res, merge_sort)
    for what in ("second", "third"):
        state, step = pair.build(what)
        _moved(step, HELD, (merge_sort, what))
        _same_state(state, first, (merge_sort, what))
    pair.close()


def _whole_calls(hip, prob, s, debug):
    """upload, then two optimizeResident calls of fixed length -> per call (poses, global points, report, trace), counters"""
    opt = hip.DmsaOptimizer(fixed_iters=True, debug=debug)
    opt.upload(prob)
    out = []
    for _ in range(2):
        r = opt.optimizeResident(s)
        rep = (r.iterations, r.stop_reason, r.evaluations, r.num_gaussians, r.num_gaussians_l1, r.num_memberships, r.error0, r.last_step_norm, r.last_line_search_k)
        tr = [(t["M"], t["M1"], t["Mm"], t["best_k"], t["error0"], t["step_norm"]) for t in opt.trace()[: r.iterations]]
        ro, rt = opt.poses()
        out.append((ro, rt, opt.globalPoints(), rep, tr))
    c = opt.debugCounters()
    opt.close()
    assert c["sync_retries"] == 0, c
    return out, c


def _same_calls(a, b, what):
    for k, ((oa, ta, ga, ra, tra), (ob, tb, gb, rb, trb)) in enumerate(zip(a, b)):
        assert ra == rb and tra == trb, (what, k, ra, rb)
        assert oa.tobytes() == ob.tobytes() and ta.tobytes() == tb.tobytes() and ga.tobytes() == gb.tobytes(), (what, k)


@pytest.mark.parametrize("name", ["window_two_sorts", "window_merged", "keyframes_8"])
def test_whole_calls(hip, name):
    """optimizeResident, 6 iterations, twice: poses, global points, report and trace against keys_ahead = 0 -- and the default, which takes the
    ahead order once eight voxelisations in a row have left the tables alone (the last builds of the second call).  keys_ahead_held > 0: the
    ahead order was taken."""
    if name == "keyframes_8":
        prob, s, extra = synth.keyframe_problem(seed=5, frames=8, rings=24, az_steps=160, arc=0.5), DmsaOptimSettings.keyframe_map(num_iter=6), {}
    else:
        prob = synth.window_problem(seed=1, scans=3, rings=16, az_steps=128, num_static=2000)  # 8 144 points
        s, extra = DmsaOptimSettings.sliding_window(num_iter=6), {"merge_sort": 0 if name == "window_two_sorts" else 1}
    off, c_off = _whole_calls(hip, prob, s, dict(PLAIN, **extra))
    on, c_on = _whole_calls(hip, prob, s, dict(AHEAD, **extra))
    default, c_default = _whole_calls(hip, prob, s, extra or None)
    print(f"{name}: keys_ahead=2 { {k: c_on[k] for k in COUNTERS} }; default { {k: c_default[k] for k in COUNTERS} }")
    assert [r[3][0] for r in off] == [6, 6]
    _same_calls(on, off, name)
    _same_calls(default, off, name)
    assert c_off["keys_ahead_held"] == 0 and c_off["keys_ahead_redone"] == 0
    assert c_on["keys_ahead_held"] > 0 and c_default["keys_ahead_held"] > 0, (c_on, c_default)
    assert c_on["keys_ahead_held"] + 2 * c_on["keys_ahead_redone"] <= 2 * 11  # every iteration but the one behind the upload can be keyed ahead
