"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs.

Bars (BASELINE.json north_star): bit-exact voxel keys / leaf order / member lists; residuals <= 1e-6 relative;
poses within 1e-4 m / 1e-4 rad after the same iteration count.  Sizes are kept where the oracle finishes in seconds.
"""
import numpy as np
import pytest

from analytic_edge_cases import branch_window as _branch_window
from dmsa_lidar_slam_amd import synth
from dmsa_lidar_slam_amd.problems import DmsaOptimSettings

pytestmark = pytest.mark.gpu

H_INCR = float(np.sqrt(np.finfo(np.float32).eps))


@pytest.fixture(scope="module")
def small_window():
    return synth.window_problem(seed=7, scans=4, rings=32, az_steps=256, num_static=8000)


@pytest.fixture(scope="module")
def imu_window():
    return synth.window_problem(seed=8, scans=3, rings=32, az_steps=192, num_static=5000, use_imu=True)


@pytest.fixture(scope="module")
def small_keyframes():
    return synth.keyframe_problem(seed=3, frames=8, rings=24, az_steps=160, arc=0.5)


def _global_points(orc, prob):
    table, _ = orc.window_pose_table(prob)
    g = orc.transform_points(table, prob.localPoints, prob.tformIdPerPoint)
    return np.concatenate([g, prob.staticPoints]).astype(np.float32), table


# ------------------------------------------------------------------------------------------------------------------
def test_pose_table_host_mode_bit_exact(hip, orc, small_window):
    opt = hip.DmsaOptimizer(pose_table_host=True)
    opt.upload(small_window)
    got = opt.poseTables(small_window.getPoseParameters())[0]
    ref, _ = orc.window_pose_table(small_window)
    assert np.array_equal(got, ref)


def test_pose_table_device_kernel(hip, orc, small_window):
    """The default path builds the dense pose tables ON THE DEVICE; with the shared operation sequences of include/dmsa_detmath.h
    they equal the oracle's bit for bit (no host tables needed for the 1e-4 bar)."""
    opt = hip.DmsaOptimizer()
    opt.upload(small_window)
    rng = np.random.default_rng(0)
    base = small_window.getPoseParameters()
    params = np.stack([base, base + rng.normal(0, 1e-3, base.shape), base + H_INCR * np.eye(len(base))[3]])
    got = opt.poseTables(params)
    for b in range(3):
        p = small_window.copy()
        c = p.numControlPoses
        p.relOrientations[1:] = params[b, :3 * (c - 1)].reshape(c - 1, 3)
        p.relTranslations[1:] = params[b, 3 * (c - 1):].reshape(c - 1, 3)
        ref, _ = orc.window_pose_table(p)
        assert np.array_equal(got[b], ref)


@pytest.mark.parametrize("C", [3, 64])
@pytest.mark.parametrize("rows", [8, 300])
def test_pose_table_device_kernel_branches(hip, orc, C, rows):
    """k_window_pose_tables at the smallest shapes that reach every branch of d_window_pose (_branch_window): the fewest control poses
    a window may have and kMaxCtrl = 64 (the LDS arrays full), 8 table rows and 300 (a second, partial 256-thread block), three parameter
    sets (blockIdx.y > 0).  Bit for bit the oracle's tables and those of the host build (pose_table_host).
    (Three control poses, not two: Floater-Hormann with d = 2 has no weights for two nodes -- the reference's interpolant throws, the
    tables would be NaN -- so the upload refuses them; asserted here.)"""
    n_t = rows - 1
    probs = _branch_window(orc, C, n_t)
    refs = [orc.window_pose_table(p)[0] for p in probs]
    assert all(np.isfinite(r).all() for r in refs)
    params = np.stack([p.getPoseParameters() for p in probs])
    got = {}
    for host in (False, True):
        opt = hip.DmsaOptimizer(pose_table_host=host)
        opt.upload(probs[0])
        got[host] = opt.poseTables(params)
        assert got[host].shape == (3, n_t, 12)
    for b in range(3):
        assert np.array_equal(got[False][b], refs[b]), (C, rows, b)
    assert np.array_equal(got[False], got[True])
    if C == 3:
        two = probs[0].copy()
        two.relOrientations, two.relTranslations, two.stamps = two.relOrientations[:2], two.relTranslations[:2], two.stamps[:2]
        with pytest.raises(hip.DmsaError):
            hip.DmsaOptimizer().upload(two)


def test_transform_bit_exact(hip, orc, small_window):
    opt = hip.DmsaOptimizer()
    opt.upload(small_window)
    opt.poseTables(small_window.getPoseParameters())
    got = opt.updateGlobalPoints(0)
    ref, _ = _global_points(orc, small_window)
    n = small_window.localPoints.shape[0]
    assert np.array_equal(got[:n, :3], ref[:n, :3])


def _stage_setup(hip, orc, prob, settings):
    opt = hip.DmsaOptimizer()
    opt.upload(prob)
    opt.poseTables(prob.getPoseParameters())
    opt.updateGlobalPoints(0, download=False)
    M, Mm = opt.buildGaussians(settings)
    glob, table = _global_points(orc, prob)
    ids = np.concatenate([prob.ringIds, prob.staticRingIds])
    return opt, glob, ids, table, M, Mm


@pytest.mark.parametrize("level", [0, 1])
def test_voxel_keys_and_leaf_order_bit_exact(hip, orc, small_window, level):
    s = DmsaOptimSettings.sliding_window()
    opt, glob, ids, _, _, _ = _stage_setup(hip, orc, small_window, s)
    factor = np.float32(s.grid_size_1_factor if level == 0 else s.grid_size_2_factor)
    res = float(factor * np.float32(small_window.minGridSize))
    info_r, code_r, key_r, order_r = orc.voxelize(glob, res)
    info, code, key, order = opt.voxelLevel(level)
    assert info.resolution == res
    assert info.depth == info_r.depth and info.num_events == info_r.num_events
    assert list(info.min_xyz) == list(info_r.min_xyz)
    assert info.num_valid == info_r.num_valid and info.num_leaves == info_r.num_leaves
    assert np.array_equal(key, key_r)
    assert np.array_equal(code, code_r)
    assert np.array_equal(order, order_r)


def test_voxel_with_nonfinite_points(hip, orc):
    prob = synth.window_problem(seed=11, scans=2, rings=16, az_steps=128, num_static=1000)
    prob.localPoints[0, 0] = np.nan          # first point NaN: lattice anchors at the next finite point
    prob.localPoints[500, 1] = np.inf
    prob.staticPoints[3, 2] = -np.inf
    s = DmsaOptimSettings.sliding_window()
    opt, glob, ids, _, _, _ = _stage_setup(hip, orc, prob, s)
    for level, f in ((0, s.grid_size_1_factor), (1, s.grid_size_2_factor)):
        res = float(np.float32(f) * np.float32(prob.minGridSize))
        info_r, code_r, key_r, order_r = orc.voxelize(glob, res)
        info, code, key, order = opt.voxelLevel(level)
        assert info.num_valid == info_r.num_valid == glob.shape[0] - 3
        assert np.array_equal(code, code_r) and np.array_equal(order, order_r)
        assert list(info.min_xyz) == list(info_r.min_xyz)


def test_gaussian_sets_bit_exact_and_info_close(hip, orc, small_window):
    s = DmsaOptimSettings.sliding_window()
    opt, glob, ids, _, M, Mm = _stage_setup(hip, orc, small_window, s)
    ref = orc.Gaussians(glob, ids, small_window.minGridSize, s)
    assert (M, Mm) == (ref.M, ref.Mm)
    seg, memb, info, w = opt.gaussians()
    assert np.array_equal(seg, ref.seg_offset)
    assert np.array_equal(memb, ref.members)
    # the fit's float reductions in Eigen's own orders on both sides: the oracle's bits
    assert np.array_equal(info, ref.info) and np.array_equal(w, ref.weights)


def test_fit_weights_and_residuals_bit_exact(hip, orc, small_window):
    """Gaussian fit, weights and residuals reproduce the oracle bit for bit (three evaluations: base, a forward difference, a far one)."""
    s = DmsaOptimSettings.sliding_window()
    opt, glob, ids, table, M, Mm = _stage_setup(hip, orc, small_window, s)
    ref = orc.Gaussians(glob, ids, small_window.minGridSize, s)
    seg, memb, info, w = opt.gaussians()
    assert np.array_equal(seg, ref.seg_offset) and np.array_equal(memb, ref.members)
    assert np.array_equal(info, ref.info)
    assert np.array_equal(w, ref.weights)
    base = small_window.getPoseParameters()
    params = np.stack([base, base + H_INCR * np.eye(len(base))[1], base - 3e-3])
    tables = opt.poseTables(params)
    e = opt.evalResiduals(3)
    for b in range(3):
        g = orc.transform_points(tables[b], small_window.localPoints, small_window.tformIdPerPoint)
        gl = np.concatenate([g, small_window.staticPoints]).astype(np.float32)
        assert np.array_equal(e[b], ref.residuals(gl))


def test_normal_equations(hip, orc, small_window):
    s = DmsaOptimSettings.sliding_window()
    opt, glob, ids, table, M, Mm = _stage_setup(hip, orc, small_window, s)
    base = small_window.getPoseParameters()
    P = len(base)
    params = np.concatenate([base[None], base[None] + H_INCR * np.eye(P)])
    opt.poseTables(params, download=False)
    e = opt.evalResiduals(P + 1)
    lam = float(np.float32(1e-5))
    H, g = opt.normalEquations(P, H_INCR, lam)
    H_ref, g_ref, step_ref = orc.lm_step(e[0], e[1:], H_INCR, lam, 0.2)
    assert np.abs(H - H_ref).max() / np.abs(H_ref).max() < 1e-12
    assert np.abs(g - g_ref).max() / np.abs(g_ref).max() < 1e-12


def test_adaptive_step_size_entry(hip, orc, small_window):
    """dmsa_adaptive_step_size = DmsaOptimizer::adaptiveStepSize (DmsaOptimizer.h:152-182, public in the reference): the arg-min over the nine
    trials 0.1 k step of e^T e, strictly below error0, from residuals the library evaluates itself -- checked against the same nine
    evaluations made through the stage calls; 0 and untouched parameters when nothing beats error0."""
    s = DmsaOptimSettings.sliding_window()
    opt, glob, ids, table, M, Mm = _stage_setup(hip, orc, small_window, s)
    base = small_window.getPoseParameters()
    P = len(base)
    params = np.concatenate([base[None], base[None] + H_INCR * np.eye(P)])
    opt.poseTables(params, download=False)
    e = opt.evalResiduals(P + 1)
    _, _, step = orc.lm_step(e[0], e[1:], H_INCR, float(np.float32(1e-5)), 0.2)
    trials = np.stack([base + 0.1 * k * step for k in range(1, 10)])
    opt.poseTables(trials, download=False)
    errs = (opt.evalResiduals(9) ** 2).sum(1)
    error0 = float((e[0] ** 2).sum())
    want = int(np.argmin(errs)) + 1 if errs.min() < error0 else 0
    got_params, k = opt.adaptiveStepSize(base, step, error0)
    assert k == want and 1 <= k <= 9
    assert np.array_equal(got_params, base + 0.1 * k * step)
    # an error0 nothing can beat: best_k = 0, parameters as they came
    got_params, k = opt.adaptiveStepSize(base, step, 0.0)
    assert k == 0 and np.array_equal(got_params, base)
    opt.close()


def _pose_diff(orc, a, b):
    ga_o, ga_t = orc.relative2global(a.relOrientations, a.relTranslations)
    gb_o, gb_t = orc.relative2global(b.relOrientations, b.relTranslations)
    return np.abs(ga_t - gb_t).max(), np.abs(ga_o - gb_o).max()


def test_optimize_window_matches_oracle(hip, orc, small_window):
    """Reference-order sums, device pose tables: poses within 1e-4 m / 1e-4 rad after the same iterations."""
    s = DmsaOptimSettings.sliding_window(num_iter=5)
    p_ref, p_gpu = small_window.copy(), small_window.copy()
    rep_ref, gl_ref, trace = orc.optimize_window(p_ref, s, want_global=True)
    opt = hip.DmsaOptimizer()
    rep = opt.optimizeSet(p_gpu, s)
    assert rep.iterations == rep_ref.iterations and rep.stop_reason == rep_ref.stop_reason
    assert rep.evaluations == rep_ref.evaluations
    tr = opt.trace()
    for a, b in zip(trace, tr):
        assert (a["M"], a["M1"], a["Mm"], a["best_k"]) == (b["M"], b["M1"], b["Mm"], b["best_k"])
        assert abs(a["error0"] - b["error0"]) <= 1e-9 * a["error0"]
    dt, dr = _pose_diff(orc, p_ref, p_gpu)
    assert dt < 1e-4 and dr < 1e-4, (dt, dr)
    gl = opt.globalPoints()
    assert np.abs(gl[:, :3] - gl_ref[:, :3]).max() < 2e-4
    moved_t, moved_r = _pose_diff(orc, small_window, p_gpu)  # the check is not vacuous
    assert moved_t > 1e-3 or moved_r > 1e-3


def test_optimize_window_with_imu_rows(hip, orc, imu_window):
    s = DmsaOptimSettings.sliding_window(use_imu=True, num_iter=4)
    p_ref, p_gpu = imu_window.copy(), imu_window.copy()
    rep_ref, _, _ = orc.optimize_window(p_ref, s)
    rep = hip.DmsaOptimizer().optimizeSet(p_gpu, s)
    assert rep.iterations == rep_ref.iterations and rep.stop_reason == rep_ref.stop_reason
    dt, dr = _pose_diff(orc, p_ref, p_gpu)
    assert dt < 1e-4 and dr < 1e-4, (dt, dr)


def test_few_gaussians_abort(hip, orc):
    prob = synth.window_problem(seed=2, scans=2, rings=4, az_steps=16, num_static=0)
    s = DmsaOptimSettings.sliding_window(num_iter=3)
    p_ref, p_gpu = prob.copy(), prob.copy()
    rep_ref, _, _ = orc.optimize_window(p_ref, s)
    rep = hip.DmsaOptimizer().optimizeSet(p_gpu, s)
    assert rep_ref.stop_reason == 1 and rep.stop_reason == 1  # DMSA_STOP_FEW_GAUSSIANS
    assert rep.iterations == rep_ref.iterations == 1
    dt, dr = _pose_diff(orc, p_ref, p_gpu)
    assert dt < 1e-12 and dr < 1e-12


# ---- keyframe model -------------------------------------------------------------------------------------------------
def test_keyframe_tables_and_split_gaussians(hip, orc, small_keyframes):
    prob = small_keyframes
    s = DmsaOptimSettings.keyframe_map()
    opt = hip.DmsaOptimizer()
    opt.upload(prob)
    tab = opt.poseTables(prob.getPoseParameters())[0]
    ref_tab = orc.keyframe_pose_table(prob)
    assert np.array_equal(tab, ref_tab)
    glob = opt.updateGlobalPoints(0)
    rows = np.repeat(np.arange(prob.numFrames, dtype=np.int32), np.diff(prob.frameOffsets))
    g_ref = orc.transform_points(ref_tab, prob.localPoints, rows)
    assert np.array_equal(glob[:, :3], g_ref[:, :3])
    # normals rotated with the 3-term x0 + (x1 + x2) order
    R = ref_tab.reshape(-1, 3, 4)[rows][:, :, :3]
    nl = prob.localNormals[:, :3]
    f = np.float32
    t = (R * nl[:, None, :]).astype(f)
    n_ref = (t[:, :, 0] + (t[:, :, 1] + t[:, :, 2]).astype(f)).astype(f)
    n4 = np.concatenate([n_ref, np.zeros((n_ref.shape[0], 1), f)], axis=1)
    M, Mm = opt.buildGaussians(s)
    ref = orc.Gaussians(g_ref, prob.ringIds, prob.minGridSize, s, normals4=n4)
    assert (M, Mm) == (ref.M, ref.Mm)
    seg, memb, info, w = opt.gaussians()
    assert np.array_equal(seg, ref.seg_offset) and np.array_equal(memb, ref.members)
    # the split really happened somewhere (a set whose members are not one contiguous leaf run)
    ref_nosplit = orc.Gaussians(g_ref, prob.ringIds, prob.minGridSize, DmsaOptimSettings(min_num_points_per_set=10), normals4=n4)
    assert ref.M != ref_nosplit.M or ref.Mm != ref_nosplit.Mm


@pytest.mark.parametrize("case", ["noisy", "duplicates", "flipped_tail"])
def test_split_pair_search_takes_only_partners_behind_a_position(hip, orc, small_keyframes, case):
    """splitSet's double loop (Gaussians.h:36-51) keeps the FIRST minimal pair in (a outer, c inner) order; k_split_pairs only looks at
    partners c > a because |n_a + n_c| has the bits of |n_c + n_a|, so that pair has a < c.  Normals that make the minimum fall anywhere:
    noise (no ties, the best partner of most members lies in front of them), exact duplicates and exact opposites (ties at the minimum,
    also with the value 0), and opposites only among the LAST members of every frame (the minimal pairs sit at the end of the leaves)."""
    prob = small_keyframes.copy()
    rng = np.random.default_rng({"noisy": 1, "duplicates": 2, "flipped_tail": 3}[case])
    f = np.float32
    nl = prob.localNormals.copy()
    n = nl.shape[0]
    if case == "noisy":
        nl[:, :3] += rng.normal(0, 0.3, (n, 3)).astype(f)
        nl[rng.random(n) < 0.35, :3] *= f(-1)
    elif case == "duplicates":
        nl[:, :3] = np.round(nl[:, :3] * f(4)) / f(4)       # a handful of distinct directions: ties everywhere
        nl[rng.random(n) < 0.5, :3] *= f(-1)                # and exact opposites: |n_a + n_c| = 0 for many pairs
        nl[(nl[:, :3] == 0).all(axis=1), 2] = 1
    else:
        for k in range(prob.numFrames):
            a, b = prob.frameOffsets[k], prob.frameOffsets[k + 1]
            nl[b - (b - a) // 5:b, :3] *= f(-1)
        nl[:, :3] += rng.normal(0, 0.02, (n, 3)).astype(f)
    nrm = np.linalg.norm(nl[:, :3].astype(np.float64), axis=1)
    nl[:, :3] = (nl[:, :3] / np.maximum(nrm, 1e-6)[:, None]).astype(f)
    prob.localNormals = nl
    s = DmsaOptimSettings.keyframe_map()
    opt = hip.DmsaOptimizer()
    opt.upload(prob)
    ref_tab = orc.keyframe_pose_table(prob)
    assert np.array_equal(opt.poseTables(prob.getPoseParameters())[0], ref_tab)
    rows = np.repeat(np.arange(prob.numFrames, dtype=np.int32), np.diff(prob.frameOffsets))
    g_ref = orc.transform_points(ref_tab, prob.localPoints, rows)
    assert np.array_equal(opt.updateGlobalPoints(0)[:, :3], g_ref[:, :3])
    R = ref_tab.reshape(-1, 3, 4)[rows][:, :, :3]
    t = (R * nl[:, None, :3]).astype(f)
    n_ref = (t[:, :, 0] + (t[:, :, 1] + t[:, :, 2]).astype(f)).astype(f)
    n4 = np.concatenate([n_ref, np.zeros((n, 1), f)], axis=1)
    M, Mm = opt.buildGaussians(s)
    ref = orc.Gaussians(g_ref, prob.ringIds, prob.minGridSize, s, normals4=n4)
    assert (M, Mm) == (ref.M, ref.Mm)
    seg, memb, info, w = opt.gaussians()
    opt.close()
    assert np.array_equal(seg, ref.seg_offset) and np.array_equal(memb, ref.members)
    ref_nosplit = orc.Gaussians(g_ref, prob.ringIds, prob.minGridSize, DmsaOptimSettings(min_num_points_per_set=10), normals4=n4)
    assert ref.M != ref_nosplit.M or ref.Mm != ref_nosplit.Mm  # leaves were split


def test_optimize_keyframes_matches_oracle(hip, orc, small_keyframes):
    s = DmsaOptimSettings.keyframe_map(num_iter=3)
    p_ref, p_gpu = small_keyframes.copy(), small_keyframes.copy()
    rep_ref, _, _ = orc.optimize_keyframes(p_ref, s)
    rep = hip.DmsaOptimizer().optimizeSet(p_gpu, s)
    assert rep.iterations == rep_ref.iterations and rep.stop_reason == rep_ref.stop_reason
    dt, dr = _pose_diff(orc, p_ref, p_gpu)
    assert dt < 1e-4 and dr < 1e-4, (dt, dr)
