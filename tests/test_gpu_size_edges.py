"""The fit and the correspondence kernels at every size-class boundary, bit for bit against the oracle.

The cloud of tests/size_edge_cloud.py has one Gaussian (at both resolutions) for every member count around every constant the kernels
branch on -- acceptance (10), the lane-per-evaluation tier (32 / 256 / small_threshold), 64 lanes, DMSA_LONG_CHUNK, every chain-bin edge
2^k and 3 * 2^(k-1), the latency tier (2^12, and 2^9 .. 2^13 through long_log2), the fit's chunks of 256 x waves members, the eight helper
workgroups, Eigen's kc and 2 kc for both L1 sizes.  tests/test_size_edge_cloud.py proves on the CPU that the cloud has these counts; the
tests here assert the same before they compare anything.  Every comparison is np.array_equal; the only tolerances are the ones
tests/test_gpu_analytic_jacobian.py already uses for the analytic Jacobian.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import size_edge_cloud as sec
from dmsa_lidar_slam_amd.problems import DmsaOptimSettings
from test_analytic_jacobian_model import jacobian_model
from test_gpu_loop import _run, _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H_INCR = float(np.sqrt(np.finfo(np.float32).eps))
BATCHES = (1, 9, 16, 17, 32, 33, 40)  # one and several sub-batches of the kBL = 16 layout, both sides of long_split's B <= 32


def _batch(base, B):
    """base parameters plus H_INCR unit perturbations (of growing length once the P parameters are used up)"""
    P = len(base)
    return np.stack([base] + [base + H_INCR * (1 + k // P) * np.eye(P)[k % P] for k in range(B - 1)])


class _Cloud:
    def __init__(self, orc, prob, s, off, counts):
        self.prob, self.s, self.off, self.counts = prob, s, off, counts
        self.first = prob.localPoints.shape[0]
        self.glob, self.ids = sec.global_points(orc, prob)
        self.ref = orc.Gaussians(self.glob, self.ids, prob.minGridSize, s)
        self.found = sec.check_clusters(self.ref, self.first, off, counts)  # the condition of every comparison below
        self.sizes = np.diff(self.ref.seg_offset)
        self.base = prob.getPoseParameters()
        self.params = _batch(self.base, max(BATCHES))
        self.tables = None
        self.e_ref = None

    def open(self, hip, debug=None):
        """a context with the cloud uploaded and its Gaussians built; the structure is the oracle's"""
        opt = hip.DmsaOptimizer(debug=debug)
        opt.upload(self.prob)
        opt.poseTables(self.base[None, :], download=False)
        opt.updateGlobalPoints(0, download=False)
        assert opt.buildGaussians(self.s) == (self.ref.M, self.ref.Mm), debug
        return opt

    def residuals(self, orc, opt, B):
        """(device residuals of the first B parameter sets, the oracle's): ref.residuals of the oracle-transformed points"""
        tables = opt.poseTables(self.params[:B])
        if self.tables is None:
            self.tables = opt.poseTables(self.params)
            self.e_ref = np.array([self.ref.residuals(np.concatenate([orc.transform_points(t, self.prob.localPoints, self.prob.tformIdPerPoint),
                                                                      self.prob.staticPoints]).astype(np.float32)) for t in self.tables])
            tables = opt.poseTables(self.params[:B])
        assert np.array_equal(tables, self.tables[:B])
        return opt.evalResiduals(B), self.e_ref[:B]

    def differing(self, e, e_ref):
        """the member counts of the Gaussians whose residuals differ (for the assertion message)"""
        bad = np.flatnonzero((e != e_ref).any(axis=0))
        return f"{bad.size} Gaussians differ, member counts {sorted(set(self.sizes[bad].tolist()))[:24]}, max |diff| {np.abs(e - e_ref).max():.3e}"


@pytest.fixture(scope="module")
def cloud(orc):
    counts = sec.count_list(orc)
    prob, s, off = sec.window(counts)
    return _Cloud(orc, prob, s, off, counts)


# ---- the fit --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l1", sec.EIGEN_L1)
def test_fit_at_every_size_boundary(hip, orc, cloud, l1):
    """seg_offset, members, the nine floats of info and the weights at both depth blockings of Eigen's product (kc 680 / 1016)."""
    try:
        orc.set_eigen_l1_bytes(l1)
        ref = orc.Gaussians(cloud.glob, cloud.ids, cloud.prob.minGridSize, cloud.s)
    finally:
        orc.set_eigen_l1_bytes(sec.EIGEN_L1[0])
    opt = cloud.open(hip, {"eigen_l1_bytes": l1})
    seg, memb, info, w = opt.gaussians()
    opt.close()
    sec.check_clusters(types.SimpleNamespace(M=len(seg) - 1, seg_offset=seg, members=memb), cloud.first, cloud.off, cloud.counts)
    assert np.array_equal(seg, ref.seg_offset) and np.array_equal(memb, ref.members)
    bad = np.flatnonzero((info != ref.info).any(axis=1) | (w != ref.weights))
    assert bad.size == 0, f"eigen_l1_bytes {l1}: fit differs for member counts {sorted(set(np.diff(seg)[bad].tolist()))}"
    assert np.array_equal(info, ref.info) and np.array_equal(w, ref.weights)
    if l1 != sec.EIGEN_L1[0]:  # the blocking matters here: Gaussians above 680 members differ between the two L1 sizes
        assert not np.array_equal(ref.info, cloud.ref.info)


# ---- residual batches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_residual_batches_at_every_size_boundary(hip, orc, cloud, B):
    opt = cloud.open(hip)
    e, e_ref = cloud.residuals(orc, opt, B)
    opt.close()
    assert np.array_equal(e, e_ref), f"B {B}: {cloud.differing(e, e_ref)}"


# ---- the switch matrix ---------------------------------------------------------------------------------------------------------------
# Crossed: small_threshold x long_log2 (both move a tier boundary of k_size_classes: 45 pairs) and serial_tree x long_split (who computes the
# second pass of a long Gaussian, and how), the latter at the built-in latency tier (18 long Gaussians: more than the 16 the automatic rule
# long_split = 1 allows, so 1 equals 0 there) and at long_log2 = 13 (4 long Gaussians: the automatic rule hands over).  Everything else one
# value at a time on the defaults.  B = 17: two sub-batches, B <= 32.
_SMALL = (0, 1, 8, 31, 32, 33, 100, 255, 256)
_LONG = (0, 9, 10, 11, 13)
_MATRIX = [{"small_threshold": st, "long_log2": ll} for st in _SMALL for ll in _LONG]
_MATRIX += [{"serial_tree": t, "long_split": sp, "long_log2": ll} for t in (0, 1, 2, 3) for sp in (0, 1, 2, 4096) for ll in (0, 13)]
_MATRIX += [{"serial_streams": n} for n in (1, 2, 3)] + [{"shared_rotations": 0}, {"eval_skip": 0}, {"eval_skip": 2, "skip_stats": 1}]


@pytest.mark.parametrize("debug", _MATRIX, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_switches_change_no_bit_at_any_size(hip, orc, cloud, debug):
    B = 17
    opt = cloud.open(hip, debug)
    seg, memb, info, w = opt.gaussians()
    assert np.array_equal(seg, cloud.ref.seg_offset) and np.array_equal(memb, cloud.ref.members)
    bad = np.flatnonzero((info != cloud.ref.info).any(axis=1) | (w != cloud.ref.weights))
    assert bad.size == 0, f"{debug}: fit differs for member counts {sorted(set(cloud.sizes[bad].tolist()))}"
    e, e_ref = cloud.residuals(orc, opt, B)
    opt.close()
    assert np.array_equal(e, e_ref), f"{debug}: {cloud.differing(e, e_ref)}"
    if debug.get("eval_skip") == 2:
        # the counters are kept by k_jacobian_columns: one iteration of a whole call on the same cloud.  (The skip logic engages above 64
        # parameters only -- optimize_loop.cpp -- so at this window's P = 30 nothing is left out and nothing can mismatch; the stage call
        # above computes every pair in every mode.)
        opt = hip.DmsaOptimizer(debug=debug)
        opt.optimizeSet(cloud.prob.copy(), DmsaOptimSettings.sliding_window(num_iter=1))
        counters = opt.debugCounters()
        opt.close()
        assert counters["skip_mismatches"] == 0, counters


# ---- adversarial members ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first_block", "middle_block", "last_block"])
def test_planted_members_at_the_size_boundaries(hip, orc, cloud, where):
    """One member of a cluster on each side of DMSA_LONG_CHUNK, of kc, of 2^12 and of 2^13 moved onto the mean of the others (the recipe of
    test_parallel_second_pass_of_the_chain_tiers): its term is ~2^-40 beside the sum, the exactness proof of the parallel second pass must
    fail and the member-by-member chain run -- in the first, a middle or the last block of the member list."""
    c = sec.constants()
    kc = sec.eigen_kc(orc)[0]
    wanted = [c["long_chunk"], c["long_chunk"] + 1, kc, kc + 1, (1 << 12) - 1, 1 << 12, (1 << 13) - 1, 1 << 13]
    prob = cloud.prob.copy()
    for n in wanted:
        i = cloud.counts.index(n)
        a = int(cloud.off[i])
        k = {"first_block": n // 50, "middle_block": n // 2, "last_block": n - 1 - n // 50}[where]
        others = np.delete(np.arange(a, a + n), k)
        prob.staticPoints[a + k, :3] = prob.staticPoints[others, :3].astype(np.float64).mean(0).astype(np.float32)
    adv = _Cloud(orc, prob, cloud.s, cloud.off, cloud.counts)  # (checks that every cluster is still one leaf with its members)
    for mode in (1, 2, 0, 3):
        opt = adv.open(hip, {"serial_tree": mode})
        opt.serialFallbackSums(reset=True)
        e, e_ref = adv.residuals(orc, opt, 9)
        fallbacks = opt.serialFallbackSums()
        opt.close()
        assert np.array_equal(e, e_ref), f"{where} serial_tree {mode}: {adv.differing(e, e_ref)}"
        if mode == 1:
            assert fallbacks > 0, where


# ---- whole calls ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole_call(orc, cloud):
    """(settings, the oracle's result) of a three-iteration optimizeSet on the constructed window"""
    s = DmsaOptimSettings.sliding_window(num_iter=3)
    p_ref = cloud.prob.copy()
    rep_ref, _, tr_ref = orc.optimize_window(p_ref, s)
    assert rep_ref.num_gaussians >= 2 * (len(cloud.counts) - 1)
    return s, (p_ref, rep_ref, tr_ref)


def test_whole_calls_on_the_constructed_window(hip, cloud, whole_call):
    s, want = whole_call
    variants = [None, {"device_loop": 0}, {"device_loop": 0, "overlap_batch": 0}, {"device_loop": 0, "overlap_batch": 1}, {"sort_prehist": 1},
                {"stream_priority": 1}, {"stream_priority": 7}, {"serial_streams": 1}, {"serial_streams": 2}, {"long_log2": 9}]
    n = cloud.prob.localPoints.shape[0] + cloud.prob.staticPoints.shape[0]
    if n <= 32768:
        variants.append({"small_voxel": 1})
    for debug in variants:
        try:
            _same(_run(hip, cloud.prob, s, debug=debug), want)
        except AssertionError as err:
            raise AssertionError(f"optimizeSet with {debug} differs from the oracle: {err}") from err


_CROSSED = [{"device_sync": ds, "dual_stream": du, "serial_streams": ss, "merge_sort": ms} for ds in (0, 1) for du in (0, 1) for ss in (1, 2, 3) for ms in (0, 1)]


@pytest.mark.parametrize("debug", _CROSSED, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_crossed_stream_variants_on_the_constructed_window(hip, cloud, whole_call, debug):
    """Every stream dependency of an iteration (csrc/dev_sync.h) in both mechanisms, counters and events, while the switches that put its
    two ends on ONE stream are crossed with it: no side stream, one / two / three tier streams (the window's 18 Gaussians of the latency
    tier make the tier fork and join real), one sort for both voxel levels or one each."""
    assert np.any(cloud.sizes >= 1 << 12)  # the latency tier (DMSA_LONG_LOG2 = 12) is not empty
    s, want = whole_call
    _same(_run(hip, cloud.prob, s, debug=debug), want)


# ---- the analytic Jacobian -----------------------------------------------------------------------------------------------------------
def test_analytic_jacobian_on_the_constructed_window(hip, cloud):
    """k_analytic_jacobian has its own member loop (4 waves): against the numpy model with the bar of tests/test_gpu_analytic_jacobian.py
    (||dJ||_F / ||J||_F <= 1e-4), its e0 against evalResiduals with that file's rtol 1e-12."""
    prob = cloud.prob
    opt = cloud.open(hip)
    M = cloud.ref.M
    P = cloud.base.size
    J, e0 = opt.analyticJacobian()
    assert J.shape == (M, P)
    seg, memb, info, w = opt.gaussians()
    dT = opt.poseTableDerivatives()
    n_t = prob.trajTime.shape[0]
    rows = np.concatenate([np.asarray(prob.tformIdPerPoint, np.int64), np.full(prob.staticPoints.shape[0], n_t)])
    x = np.concatenate([prob.localPoints[:, :3], prob.staticPoints[:, :3]])
    pg = opt.updateGlobalPoints(0)
    Jm = jacobian_model(np.concatenate([dT, np.zeros((1, 12, P))]), seg, memb, info, w, x, rows, pg, id_row=n_t)
    r_model = float(np.linalg.norm(J - Jm) / np.linalg.norm(Jm))
    print(f"[size edges] analytic Jacobian vs model {r_model:.3e} (bar 1e-4)")
    assert r_model <= 1e-4
    opt.poseTables(cloud.base[None, :], download=False)
    E = opt.evalResiduals(1)
    opt.close()
    bad = np.flatnonzero(~np.isclose(e0[:M], E[0], rtol=1e-12, atol=0))
    assert bad.size == 0, f"e0 of the analytic kernel differs for member counts {sorted(set(cloud.sizes[bad].tolist()))}"


# ---- the splitSet search at constructed leaf populations -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["noisy", "duplicates", "flipped_tail"])
def test_split_search_at_constructed_leaf_populations(hip, orc, case):
    """Leaves of 63 .. 65, kSplitChunk +- 1, kSplitChunk + 64 +- 1, kSplitBigLeaf +- 1 and around kSplitChunk x kSplitMaxChunks = 16 384 members
    -- the partner range from which k_split_tasks makes its (64-aligned) chunks wider than kSplitChunk -- and the smallest leaves with halves
    of 9, 10, 11 and 12 members (strict '>' on the halves)."""
    prob, s, off, leaves = sec.keyframes(case)
    assert s.gauss_split
    tab, g, n4 = sec.keyframe_global(orc, prob)
    ref = orc.Gaussians(g, prob.ringIds, prob.minGridSize, s, normals4=n4)
    ref0 = orc.Gaussians(g, prob.ringIds, prob.minGridSize, DmsaOptimSettings(min_num_points_per_set=sec.MIN_POINTS), normals4=n4)
    sec.check_split(ref, ref0, off, leaves)
    assert (ref.M, ref.Mm) != (ref0.M, ref0.Mm)  # the leaves really were split
    opt = hip.DmsaOptimizer(debug={"skip_stats": 1})
    opt.upload(prob)
    assert np.array_equal(opt.poseTables(prob.getPoseParameters())[0], tab)
    assert np.array_equal(opt.updateGlobalPoints(0)[:, :3], g[:, :3])
    M, Mm = opt.buildGaussians(s)
    seg, memb, _, _ = opt.gaussians() if (M, Mm) == (ref.M, ref.Mm) else (None, None, None, None)
    blocks = opt.debugCounters()["split_blocks"]
    opt.close()
    assert (M, Mm) == (ref.M, ref.Mm), case
    bad = np.flatnonzero(seg != ref.seg_offset)
    assert bad.size == 0, f"{case}: seg_offset differs from Gaussian {bad[:1]} on, oracle sizes there {np.diff(ref.seg_offset)[max(int(bad[0]) - 1, 0):int(bad[0]) + 2]}"
    assert np.array_equal(seg, ref.seg_offset) and np.array_equal(memb, ref.members)
    assert blocks > 0


# ---- the sort's tile sizes -------------------------------------------------------------------------------------------------------------
def test_radix_sort_with_every_tile_size():
    """sort_items through DMSA_DEBUG, which every context of a process reads: the comparisons of tests/test_gpu_voxel_prims.py (32- and 64-bit
    keys, sizes around 512 x items) in a fresh child process per tile size -- 8 is an instantiation the by-size rule (2, 4, 16) never picks.  One child after the other, each with its
    own time limit; the first one that fails ends the test."""
    for items in (2, 4, 8, 16):
        env = dict(os.environ, DMSA_DEBUG=f"sort_items={items}")
        cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_voxel_prims.py"), "-q", "-x", "-m", "gpu", "-k", "radix_sort",
               "-p", "no:cacheprovider"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, f"sort_items={items}:\n" + r.stdout[-3000:] + r.stderr[-2000:]
        assert " passed" in r.stdout and "skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-1000:]
