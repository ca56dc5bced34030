"""Keyframe passes above 192 parameters, whole optimizeSet calls against the oracle bit for bit.

optimize_device_loop (csrc/optimize_loop.cpp) changes paths by P: one-workgroup LM step (P <= 64), stream of pivot-step records
(<= 192), column-block panels (k_loop_lm_panels, <= kLoopPanelMaxP = 1024), host solve after a synchronisation beyond.  Above 64 the
Jacobian batch leaves out the (Gaussian, evaluation) pairs that equal evaluation 0 (eval_skip) and the normal equations run on the
matrix cores with a ragged last 32-wide tile.  Covered here: the reference's own loop-closure pass (the last 100 keyframes of a map,
P = 594, 604 evaluations per iteration), its everyday 4- and 5-frame submaps, the P on both sides of each solver boundary, the stages of
iteration 0 at P = 198 / 594 / 1020 (to localise a failure of the whole calls), and one context that moves between pass sizes.

The oracle runs evaluation-parallel (orc.set_threads): bit-identical to one thread for keyframe sets
(tests/test_oracle_math.py::test_parallel_baseline_variant).
"""
import math
import os
import time

import numpy as np
import pytest

import ne_bound
from dmsa_lidar_slam_amd import synth
from dmsa_lidar_slam_amd.api import DmsaError
from dmsa_lidar_slam_amd.problems import DmsaOptimSettings

pytestmark = pytest.mark.gpu

# the forward-difference increment of the reference and of the loop: sqrt taken in double (np.sqrt of the float32 eps would round it to
# float, 0.00034526697709 instead of 0.00034526698300, and no Jacobian column would keep the dump's bits)
H_INCR = math.sqrt(float(np.finfo(np.float32).eps))
THREADS = min(16, int(os.environ.get("OMP_NUM_THREADS", "16")))


# ---- problems and runs -----------------------------------------------------------------------------------------------------------------
def _light(frames: int):
    """~380 points with normals per frame on the reference map's ring path (2 pi / 256 per frame), gravity rows: P = 6 (frames - 1)."""
    return synth.keyframe_problem(frames=frames, rings=8, az_steps=48, arc=2 * np.pi * frames / 256.0)


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            if name.startswith("map"):  # the reference's map: ~10^4 points per frame; the loop closure optimises fromId = 30 .. newest = 129
                if "map" not in cache:
                    cache["map"] = synth.keyframe_problem(frames=130, arc=2 * np.pi * 130 / 256.0)
                lo, hi = {"map_loop_closure": (30, 129), "map_P18": (126, 129), "map_P24": (125, 129)}[name]
                cache[name] = cache["map"].getSubmap(lo, hi)
            else:
                cache[name] = _light(int(name.split("_")[1]))
        return cache[name]

    return get


@pytest.fixture(scope="module")
def oracle(orc):
    """(problems, problem name, num_iter) -> the oracle's (poses, report, trace), each run once per module."""
    cache = {}

    def run(problems, name, num_iter):
        key = (name, num_iter)
        if key not in cache:
            p = problems(name).copy()
            t0 = time.perf_counter()
            orc.set_threads(THREADS)
            try:
                rep, _, tr = orc.optimize_keyframes(p, DmsaOptimSettings.keyframe_map(num_iter=num_iter))
            finally:
                orc.set_threads(1)
            print(f"[oracle] {name} P={p.numParams} {num_iter} iterations: {time.perf_counter() - t0:.1f} s on {THREADS} threads")
            cache[key] = (p, rep, tr)
        return cache[key]

    return run


def _run(hip, prob, s, debug=None, opt=None):
    p = prob.copy()
    own = opt is None
    if own:
        opt = hip.DmsaOptimizer(debug=debug)
    rep = opt.optimizeSet(p, s)
    out = (p, rep, opt.trace())
    if own:
        opt.close()
    return out


def _same(a, b):
    """The contract of tests/test_gpu_loop.py: report, per-iteration trace and poses bit for bit."""
    (pa, ra, ta), (pb, rb, tb) = a, b
    assert (ra.iterations, ra.stop_reason, ra.evaluations, ra.num_gaussians, ra.num_gaussians_l1, ra.num_memberships) == \
           (rb.iterations, rb.stop_reason, rb.evaluations, rb.num_gaussians, rb.num_gaussians_l1, rb.num_memberships)
    assert (ra.error0, ra.last_step_norm, ra.last_line_search_k) == (rb.error0, rb.last_step_norm, rb.last_line_search_k)
    assert [(t["M"], t["M1"], t["Mm"], t["best_k"], t["error0"], t["step_norm"]) for t in ta[: ra.iterations]] == \
           [(t["M"], t["M1"], t["Mm"], t["best_k"], t["error0"], t["step_norm"]) for t in tb[: rb.iterations]]
    assert np.array_equal(pa.relOrientations, pb.relOrientations) and np.array_equal(pa.relTranslations, pb.relTranslations)


def _with_skip_stats(hip, prob, s, debug):
    opt = hip.DmsaOptimizer(debug=dict(debug, skip_stats=1))
    out = _run(hip, prob, s, opt=opt)
    c = opt.debugCounters()
    opt.close()
    return out, c


# ---- 1. the reference's loop-closure pass --------------------------------------------------------------------------------------------
def test_loop_closure_pass_of_100_keyframes(hip, problems, oracle):
    """last_n_keyframes_for_optim = 100: one optimizeSet over keyframes 30 .. 129 of a 130-frame map, P = 594, 1 + P + 9 = 604
    evaluations per iteration, ~10^4 points per frame, gauss_split and gravity rows.  The panel solve in a loop, eval_skip row ranges over
    595 evaluations, the matrix-core normal equations with 595 columns, 595 evaluations in 16-lane sub-batches: all against the oracle."""
    prob = problems("map_loop_closure")
    s = DmsaOptimSettings.keyframe_map(num_iter=2)
    assert prob.numParams == 594 and prob.localPoints.shape[0] > 900_000
    assert s.gauss_split and prob.useGravityErrorTerms
    ref = oracle(problems, "map_loop_closure", 2)
    dev = _run(hip, prob, s)
    _same(dev, ref)
    assert dev[1].iterations == 2 and dev[1].evaluations == 2 * 604
    # the submap's first frame is the anchor, not a parameter; the others moved
    assert np.array_equal(dev[0].relOrientations[0], prob.relOrientations[0]) and np.array_equal(dev[0].relTranslations[0], prob.relTranslations[0])
    assert not np.array_equal(dev[0].relTranslations[1:], prob.relTranslations[1:])
    _same(dev, _run(hip, prob, s, debug={"eval_skip": 0}))
    _same(dev, _run(hip, prob, s, debug={"device_loop": 0}))
    both, c2 = _with_skip_stats(hip, prob, s, {"eval_skip": 2})
    _same(dev, both)
    skip, c1 = _with_skip_stats(hip, prob, s, {})
    _same(dev, skip)
    assert c1["skip_pairs"] == c2["skip_pairs"] == sum(t["M"] for t in ref[2][:2]) * 594
    assert c1["skip_pairs_equal"] == c2["skip_pairs_equal"] > 0.1 * c1["skip_pairs"], c1
    assert c1["skip_mismatches"] == 0 and c2["skip_mismatches"] == 0
    print(f"[eval_skip] P=594: {c1['skip_pairs_equal']} of {c1['skip_pairs']} pairs left out "
          f"({100.0 * c1['skip_pairs_equal'] / c1['skip_pairs']:.1f} %)")


# ---- 2. the everyday submaps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,P", [("map_P18", 18), ("map_P24", 24)])
def test_everyday_submap_passes(hip, problems, oracle, name, P):
    """The newest 4 / 5 keyframes of the same map with the reference's num_iter = 50: the device-side early exits included."""
    prob = problems(name)
    assert prob.numParams == P
    ref = oracle(problems, name, 50)
    _same(_run(hip, prob, DmsaOptimSettings.keyframe_map(num_iter=50)), ref)
    print(f"[everyday] P={P}: {ref[1].iterations} iterations, stop reason {ref[1].stop_reason}")


# ---- 3. the LM solver boundaries inside whole calls ------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,P", [(33, 192), (34, 198), (171, 1020), (172, 1026)],
                         ids=["P192_last_stream", "P198_first_panels", "P1020_last_panels", "P1026_first_host"])
def test_lm_solver_boundaries_inside_whole_calls(hip, problems, oracle, frames, P):
    name = f"light_{frames}"
    prob = problems(name)
    assert prob.numParams == P
    iters = 2 if P <= 198 else 1  # (the oracle needs ~30 s per iteration at P ~ 1020 on 8 threads)
    ref = oracle(problems, name, iters)
    assert ref[1].iterations == iters
    dev = _run(hip, prob, DmsaOptimSettings.keyframe_map(num_iter=iters))
    _same(dev, ref)
    s2 = DmsaOptimSettings.keyframe_map(num_iter=2)
    dev2 = dev if iters == 2 else _run(hip, prob, s2)
    assert dev2[1].iterations == 2
    _same(dev2, _run(hip, prob, s2, debug={"device_loop": 0}))
    if P == 192:  # the stream (default) and the panels
        _same(dev2, _run(hip, prob, s2, debug={"lm_stream": 0}))
    both, c = _with_skip_stats(hip, prob, s2, {"eval_skip": 2})
    _same(dev2, both)
    assert c["skip_mismatches"] == 0 and c["skip_pairs_equal"] > 0, c


# ---- 4. the stages of iteration 0 ------------------------------------------------------------------------------------------------------
def _extra(opt, params):
    opt.setPoseParameters(params)
    return opt.getAdditionalErrorTerms()


@pytest.mark.parametrize("frames,P", [(34, 198), (100, 594), (171, 1020)])
def test_stages_of_iteration_0_at_large_p(hip, orc, problems, tmp_path, frames, P):
    """Iteration 0 stage by stage (orc.stage_dump) against the stage seam: Gaussians, the 1 + P residual evaluations with their additional
    rows, the Jacobian columns (e_k - e0) (1/h), H / g of the matrix-core normal equations (and the fp64 bound of tests/ne_bound.py), the
    panel solve's step.  The first stage that differs localises a failure of the whole-call tests above."""
    prob = problems(f"light_{frames}")
    assert prob.numParams == P
    s = DmsaOptimSettings.keyframe_map(num_iter=1)
    lam = float(np.float32(s.lambda_diag))
    orc.set_threads(THREADS)
    try:
        d = orc.stage_dump(prob, s, str(tmp_path / f"stages_P{P}.bin"))
    finally:
        orc.set_threads(1)
    a = d["a"]
    assert d["P"] == P and a == frames  # the gravity rows

    opt = hip.DmsaOptimizer()
    opt.upload(prob)
    base = prob.getPoseParameters()
    opt.poseTables(base, download=False)
    opt.updateGlobalPoints(0, download=False)
    M, Mm = opt.buildGaussians(s)
    assert (M, Mm) == (d["M"], d["Mm"])
    seg, memb, info, w = opt.gaussians()
    assert np.array_equal(seg, d["seg_offset"]) and np.array_equal(memb, d["members"])
    assert np.array_equal(info, d["info"]) and np.array_equal(w, d["weights"])

    params = np.concatenate([base[None], base[None] + H_INCR * np.eye(P)])
    opt.poseTables(params, download=False)
    e = opt.evalResiduals(P + 1)
    x = np.stack([_extra(opt, p) for p in params])
    assert x.shape == (P + 1, a)
    E = np.concatenate([e, x], axis=1)  # evaluation k: [Gaussian rows; additional rows]
    assert np.array_equal(E[0], d["error_vec"])
    J = ne_bound.jacobian(E[0], E[1:], H_INCR)
    assert J.shape == d["jacobian"].shape == (M + a, P)
    bad = np.flatnonzero(np.any(J != d["jacobian"], axis=0))
    assert bad.size == 0, f"Jacobian columns {bad[:8].tolist()} (of {bad.size}) differ"

    H, g = opt.normalEquations(P, H_INCR, lam, x)
    H_o, g_o, step_o = orc.lm_step_from_jacobian(d["error_vec"], d["jacobian"], lam, s.step_length_optim)
    assert np.array_equal(H_o, d["H"]) and np.array_equal(step_o, d["step_raw"])  # (the dump holds no g: the oracle's statements give it)
    bad = np.argwhere(H != d["H"])
    assert bad.size == 0, f"H differs at {bad[:8].tolist()} (of {len(bad)})"
    assert np.array_equal(g, g_o), np.flatnonzero(g != g_o)[:8]
    assert ne_bound.check(H, g, lam, E[0], E[1:], H_INCR) <= 1.0
    # seam rules: [J | e0] was formed in place of the residual batch
    with pytest.raises(DmsaError, match="consumed"):
        opt.normalEquations(P, H_INCR, lam, x)
    opt.evalResiduals(P + 1, download=False)
    H2, g2 = opt.normalEquations(P, H_INCR, lam, x)
    assert np.array_equal(H2, H) and np.array_equal(g2, g)

    # the device LM solve (the panels at every P here) on that system: the raw step, then the clamp to max_step
    step, nan = opt.lmSolveDevice(H, g, s.step_length_optim)
    assert not nan and np.array_equal(step, d["step_raw"]), np.abs(step - d["step_raw"]).max()
    step, nan = opt.lmSolveDevice(H, g, s.step_length_optim, s.max_step)
    assert not nan and np.array_equal(step, d["step"])
    opt.close()


# ---- 5. one context across pass sizes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lm_stream", [1, 0])
def test_one_context_across_pass_sizes(hip, problems, lm_stream):
    """A SLAM run alternates small passes with loop closures on the same optimizer.  One context through P = 594 -> 18 -> 1026 -> 186 ->
    594: each call gives the bits of a fresh context (panel_P / panel_epoch resets, d_Hp / h_Hp growth, d_skip_stats sizing, d_tables reuse,
    the chain kernels' LDS attribute).  lm_stream = 0 sends P = 186 through the panel solve too."""
    s = DmsaOptimSettings.keyframe_map(num_iter=2)
    seq = ["light_100", "map_P18", "light_172", "light_32", "light_100"]
    assert [problems(n).numParams for n in seq] == [594, 18, 1026, 186, 594]
    debug = {"lm_stream": lm_stream}
    fresh = {n: _run(hip, problems(n), s, debug=debug) for n in dict.fromkeys(seq)}
    opt = hip.DmsaOptimizer(debug=debug)
    for n in seq:
        _same(_run(hip, problems(n), s, opt=opt), fresh[n])
    opt.close()
