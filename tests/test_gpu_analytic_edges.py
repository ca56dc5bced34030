"""The analytic Jacobian per row at chunk, run and identity edges: k_window_pose_table_deriv / k_keyframe_pose_table_deriv
(csrc/dmsa_kernels.hip) and k_analytic_jacobian (csrc/analytic_jacobian.hip) on the cases of tests/analytic_edge_cases.py
(tests/test_analytic_edge_cases.py shows on the CPU that the cases are what they claim and that the bound has teeth).

Bars, and what an MI355X measures (printed with -s):
  * Gaussian rows vs the long double model on the library's own dT, Gaussians and float global points, ENTRY BY ENTRY within
    analytic_edge_cases.row_bound: gamma(c) |scale_g| S_abs[g, k] with c = L + F + 30 + (9 + L / 2) kappa_g (derivation: that module's
    docstring; with the synthetic information matrices of the CPU test c runs from 41.6 to 175.3 on these cases).  Largest error / bound:
        window C = 12 (P = 66, all patterns) 0.033    C = 3 (P = 12) 0.013    C = 64 (P = 378) 0.018
        keyframes F = 71 (P = 420) 0.016    F = 341 (P = 2040) 0.013    near-identity window 0.022, keyframes 0.033
    The static-only Gaussian's row is bit-zero; e0 equals evalResiduals(1); a second call returns the same bytes.
  * P = 2040 = kAnalyticJacobianMaxP (341 frames, one member per frame, six chunks of distinct rows, 65 280 bytes of dynamic LDS): the same
    comparison; dT against the scipy model for the six parameters of the first, a middle and the last frame.  P = 2046: refused by
    optimizeSet with the flag and by both stage calls, the numeric path runs.
  * table derivatives vs the scipy models, max abs error <= 1e-7 * max(1, |dT|max) (generic poses measure 1.5e-10 / 7.0e-10):
        branch windows (C x rows x set)   2e-11 .. 3.4e-10; before the derivative side lost the identity cut: 0.50 .. 1.00 (sets 0 and 2:
                                          control rotation 0 below 1e-5, rotation 1 its copy) and 3.4e-6 .. 1.9e-5 (set 1: the chain's cut rotation 0)
        sweep, window                     2.4e-11 .. 3.0e-11 at every s; before: 0.48, 0.45, 0.37, 0.46 at s = 1e-7, 3e-6, 8e-6, 1.2e-5 (entries ~ 1)
        sweep, keyframes                  1.7e-11 at every s; before: 0.50, 0.44, 0.40, 0.42 at the same four
        keyframes F = 341, frames 1, 170, 340   2.8e-10
    At C = 64 the scipy model (minutes of Python for all 378 parameters) is differenced for the parameters of poses 1, 2, C / 2, C - 2 and
    C - 1 only, all rows.
  * near-identity poses, analytic rows vs central differences of the library's own residuals at sqrt(FLT_EPSILON), rotation and
    translation columns separately, ||dJ||_F / ||J||_F <= 5e-2:
        window: rotation 1.2e-2, translation 7.7e-4; keyframes: rotation 8.5e-3, translation 3.5e-4
        (before the fix the rotation columns were 0.25 away on the keyframes: half of every rotation column of those poses was missing).
"""
import dataclasses
import types

import numpy as np
import pytest

import analytic_edge_cases as aec
import size_edge_cloud as sec
from dmsa_lidar_slam_amd.problems import ContinuousTrajectory
from test_analytic_jacobian_model import keyframe_table, params_to_relative, window_table

pytestmark = pytest.mark.gpu

H_INCR = aec.H_INCR

RUN_CASES = {
    "window_C12": lambda orc: aec.run_window(orc, 12),
    "window_C3": lambda orc: aec.run_window(orc, 3, full=False),
    "window_C64": lambda orc: aec.run_window(orc, 64, full=False),
    "keyframes_F71": lambda orc: aec.run_keyframes(orc, 71),
    "keyframes_F341": lambda orc: aec.run_keyframes(orc, 341),
}


def _table_model(prob):
    ro, rt = prob.relOrientations, prob.relTranslations
    if isinstance(prob, ContinuousTrajectory):
        return lambda th: window_table(*params_to_relative(ro, rt, th), prob.stamps, prob.trajTime)
    return lambda th: keyframe_table(*params_to_relative(ro, rt, th))


def _open(hip, case):
    """upload, poseTables, updateGlobalPoints, buildGaussians; the library's Gaussians hold every cluster exactly (the CONDITION)"""
    opt = hip.DmsaOptimizer()
    opt.upload(case.prob)
    opt.poseTables(case.prob.getPoseParameters(), download=False)
    opt.updateGlobalPoints(0, download=False)
    opt.buildGaussians(case.settings)
    seg, memb, info, w = opt.gaussians()
    found = aec.check_member_sets(seg, memb, case)
    if case.counts:
        sec.check_clusters(types.SimpleNamespace(M=len(seg) - 1, seg_offset=seg, members=memb), case.first, case.off, case.counts)
    return opt, (seg, memb, info, w), found


def _rows_vs_model(opt, case, gauss, found):
    """(J, e0, reference of the cluster Gaussians, their indices, dT): the library's rows and the long double model of the same inputs"""
    seg, memb, info, w = gauss
    J, e0 = opt.analyticJacobian()
    dT = opt.poseTableDerivatives()
    pg = opt.updateGlobalPoints(0)
    rows, x = case.point_rows()
    gs = [g for i in sorted(found) for g in found[i]]
    for g in gs:
        assert aec.mean_is_exact(pg[memb[seg[g]:seg[g + 1]], :3])
    dT_full = np.concatenate([dT, np.zeros((1, 12, dT.shape[2]))])
    ref = aec.jacobian_rows_ld(dT_full, seg, memb, info, w, x, rows, pg, case.id_row, gs)
    return J, e0, ref, gs, dT


def _check_rows(hip, orc, name):
    case = RUN_CASES[name](orc)
    opt, gauss, found = _open(hip, case)
    M, P = gauss[0].size - 1, case.prob.numParams
    J, e0, ref, gs, dT = _rows_vs_model(opt, case, gauss, found)
    assert J.shape == (M, P) and np.isfinite(J).all()
    err = np.abs(J[gs].astype(aec.LD) - ref["J"]).astype(np.float64)
    bound = aec.row_bound(ref)
    worst = aec.worst_ratio(J[gs], ref)
    per = {}
    for i in sorted(found):
        k = [gs.index(g) for g in found[i]]
        per[case.pats[i][0]] = aec.worst_ratio(J[gs][k], {key: v[k] for key, v in ref.items()})
    print(f"[analytic edges] {name}: M {M} P {P}: largest error / bound {worst:.3f} (`{max(per, key=per.get)}`)")
    bad = np.argwhere(err > bound)
    assert bad.size == 0, f"{name}: {len(bad)} entries outside the bound, first: Gaussian {gs[bad[0][0]]} column {bad[0][1]} error {err[tuple(bad[0])]:.3e} bound {bound[tuple(bad[0])]:.3e}; per pattern {per}"
    for i, (pname, r) in enumerate(case.pats):
        if (r == aec.STATIC).all():
            for g in found[i]:
                assert J[g].tobytes() == np.zeros(P).tobytes(), pname  # bit-zero, +0.0 in every column
    # e0 is evaluation 0 of the residual kernels; the call is reproducible to the byte
    opt.poseTables(case.prob.getPoseParameters(), download=False)
    E = opt.evalResiduals(1)
    assert np.allclose(e0[:M], E[0], rtol=1e-12, atol=0)
    J2, e02 = opt.analyticJacobian()
    assert J2.tobytes() == J.tobytes() and e02.tobytes() == e0.tobytes()
    return case, opt, dT


# ---- rows -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["window_C12", "window_C3", "window_C64", "keyframes_F71"])
def test_rows_entry_by_entry_within_the_derived_bound(hip, orc, name):
    case, opt, _ = _check_rows(hip, orc, name)
    opt.close()


def test_rows_and_table_derivatives_at_the_parameter_limit(hip, orc):
    """P = 2040: the rows as above; dT against the scipy model for the first, a middle and the last frame's six parameters."""
    case, opt, dT = _check_rows(hip, orc, "keyframes_F341")
    opt.close()
    prob = case.prob
    F, P = prob.numFrames, prob.numParams
    assert P == 2040 and dT.shape == (F, 12, P)
    cols = [3 * (f - 1) + a + half for f in (1, F // 2, F - 1) for half in (0, P // 2) for a in range(3)]
    ref = aec.table_derivatives_cols(_table_model(prob), prob.getPoseParameters(), cols)
    bar = 1e-7 * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(dT[:, :, cols] - ref).max())
    print(f"[analytic edges] keyframes_F341: table derivatives of frames 1, {F // 2}, {F - 1}: max abs error {err:.3e}, bar {bar:.3e}")
    assert err <= bar


def test_one_frame_more_is_refused_and_the_numeric_path_runs(hip, orc):
    case = aec.run_keyframes(orc, 342)
    assert case.prob.numParams == 2046
    opt, _, _ = _open(hip, case)
    for call in (opt.poseTableDerivatives, opt.analyticJacobian):
        with pytest.raises(hip.DmsaError) as ei:
            call()
        assert "2046" in str(ei.value) and "2040" in str(ei.value)
    opt.close()
    s = dataclasses.replace(case.settings, num_iter=1, min_num_gaussians=1)
    opt = hip.DmsaOptimizer()
    with pytest.raises(hip.DmsaError) as ei:
        opt.optimizeSet(case.prob.copy(), dataclasses.replace(s, use_analytic_jacobi=True))
    assert "2046" in str(ei.value) and "2040" in str(ei.value)
    rep = opt.optimizeSet(case.prob.copy(), s)
    opt.close()
    assert rep.iterations == 1 and rep.evaluations >= 1 + 2046 and rep.stop_reason != 1  # (1: too few Gaussians)


# ---- table derivatives ----------------------------------------------------------------------------------------------------------------------
def _table_error(hip, prob, settings, cols=None):
    opt = hip.DmsaOptimizer()
    opt.upload(prob)
    opt.poseTables(prob.getPoseParameters(), download=False)
    opt.updateGlobalPoints(0, download=False)
    M, _ = opt.buildGaussians(settings)
    assert M > 0  # the stage call wants Gaussians
    dT = opt.poseTableDerivatives()
    opt.close()
    cols = list(range(prob.numParams)) if cols is None else cols
    ref = aec.table_derivatives_cols(_table_model(prob), prob.getPoseParameters(), cols)
    assert dT[:, :, cols].shape == ref.shape
    return float(np.abs(dT[:, :, cols] - ref).max()), 1e-7 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("C", [3, 64])
@pytest.mark.parametrize("rows", [8, 300])
def test_table_derivatives_on_every_branch_of_the_window_pose(hip, orc, C, rows):
    from dmsa_lidar_slam_amd.problems import DmsaOptimSettings

    probs = aec.branch_window(orc, C, rows - 1)
    cols = None
    if C > 12:
        cols = [3 * (c - 1) + a + half for c in (1, 2, C // 2, C - 2, C - 1) for half in (0, probs[0].numParams // 2) for a in range(3)]
    out = []
    for b, p in enumerate(probs):
        err, bar = _table_error(hip, aec.with_static_clusters(p), DmsaOptimSettings.sliding_window(), cols)
        print(f"[analytic edges] branch window C {C} rows {rows} set {b}: table derivatives max abs error {err:.3e}, bar {bar:.3e}")
        out.append((b, err, bar))
    assert all(err <= bar for _, err, bar in out), out


@pytest.mark.parametrize("s", aec.SWEEP)
@pytest.mark.parametrize("model", ["window", "keyframes"])
def test_table_derivatives_through_the_identity_cut(hip, orc, model, s):
    """Relative rotations s * (1, -0.7, 0.4): dT is the derivative of the smooth tables at every point of the sweep."""
    from dmsa_lidar_slam_amd.problems import DmsaOptimSettings

    if model == "window":
        prob, settings = aec.sweep_window_problem(s), DmsaOptimSettings.sliding_window()
    else:
        prob, settings = aec.sweep_keyframes_problem(orc, s), DmsaOptimSettings.keyframe_map()
    err, bar = _table_error(hip, prob, settings)
    print(f"[analytic edges] sweep {model} s {s:g}: table derivatives max abs error {err:.3e}, bar {bar:.3e}")
    assert err <= bar


# ---- near-identity poses against the library's own numeric Jacobian -------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["window", "keyframes"])
def test_near_identity_rows_vs_central_differences_of_the_residuals(hip, orc, model):
    case = aec.near_identity_window(orc) if model == "window" else aec.near_identity_keyframes(orc)
    opt, gauss, found = _open(hip, case)
    J, e0, ref, gs, _ = _rows_vs_model(opt, case, gauss, found)
    theta = case.prob.getPoseParameters()
    P = theta.size
    worst = aec.worst_ratio(J[gs], ref)
    opt.poseTables(np.concatenate([theta + H_INCR * np.eye(P), theta - H_INCR * np.eye(P)]), download=False)
    Ec = opt.evalResiduals(2 * P)
    opt.close()
    Jc = ((Ec[:P] - Ec[P:]) * (0.5 / H_INCR)).T
    fro = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    M = gauss[0].size - 1
    r_rot, r_tr = fro(J[:M, :P // 2], Jc[:, :P // 2]), fro(J[:M, P // 2:], Jc[:, P // 2:])
    print(f"[analytic edges] near-identity {model}: rows vs model, largest error / bound {worst:.3f}; vs central differences of the residuals: "
          f"rotation columns {r_rot:.3e}, translation columns {r_tr:.3e} (bar 5e-2)")
    assert worst <= 1.0
    assert r_rot <= 5e-2
    assert r_tr <= 5e-2
