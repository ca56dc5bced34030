"""Debug switch ne_triangle (csrc/dmsa_kernels.hip): up to 64 parameters the normal equations compute the block sums of the elements i <= j
only (k_normal_eq_source: one workgroup per row block and tile pair, operands staged once, 2 x 2 outputs per thread), and the consumer -- the LM
step's loader in the device loop, k_normal_eq_reduce_upper in the stage call and the host-driven loop -- adds half as many block sums and gives
(j, i) the bits of (i, j).  With 0 k_normal_eq_partial computes the full square.  Every output is the same chain of the same products in the
same order, so everything here compares bit patterns (uint64 views: NaNs count too), switch 1 against 0, and against a numpy restatement of
the order: per block of 256 rows c = c + a * b row by row in float64, the block sums added in block order from 0.0.

a * b and b * a round alike, but when both factors are NaNs of different sign the product takes the first one's: with a NaN in e0 the
forward-difference columns hold its negation, and the full square is then NOT symmetric in its NaN signs.  The new form runs the twin's chain
on its own for exactly those elements; the NaN cases below check it.

Against numpy the bit patterns are compared wherever the value is not a NaN, and the NaN positions must agree: a NaN that an operation
GENERATES (inf - inf, 0 * inf) has the sign the platform gives it (set on x86, clear on the device), which is no property of the summation.
Between the two forms on the device NaNs are compared bit by bit like everything else.

The squared sums of the line search are not tested here: their kernel is the parent's (adding their block sums where they are produced was
measured and left out, docs/experiments.md round 20); tests/test_gpu_ne_wide.py runs it, and the normal equations above 64 parameters, on
caller data."""
import numpy as np
import pytest

from dmsa_lidar_slam_amd import synth
from dmsa_lidar_slam_amd.problems import DmsaOptimSettings

pytestmark = pytest.mark.gpu

ON, OFF = {"ne_triangle": 1}, {"ne_triangle": 0}
ROWS = (1, 31, 32, 33, 255, 256, 257, 511, 512, 513, 769)
PARAMS = (1, 2, 7, 30, 31, 32, 33, 63, 64)
BLOCK = 256
STOP_NO_IMPROVEMENT = 3  # include/dmsa_hip.h: dmsa_stop_reason


@pytest.fixture(scope="module")
def forms(hip):
    """one context per form, kept for the whole module"""
    on, off = hip.DmsaOptimizer(debug=ON), hip.DmsaOptimizer(debug=OFF)
    yield on, off
    on.close()
    off.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), what


def _same_as_numpy(got, ref, what):
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(_bits(got)[~nan], _bits(ref)[~nan]), what


def _columns(E, h, formed):
    """[J | e0] as the kernels form it: column k = inv_h * (E[k + 1] - E[0]), column P = E[0]; formed: E[k + 1] and E[0] as they are"""
    if formed:
        return np.concatenate([E[1:], E[:1]])
    inv_h = 1.0 / h
    return np.concatenate([inv_h * (E[1:] - E[0]), E[:1]])


def _numpy_normal_equations(E, h, formed):
    with np.errstate(all="ignore"):
        A = _columns(E, h, formed)
        n1, rows = A.shape
        Hp = np.zeros((n1, n1))
        for r0 in range(0, rows, BLOCK):
            c = np.zeros((n1, n1))
            for r in range(r0, min(rows, r0 + BLOCK)):
                c = c + A[:, r, None] * A[None, :, r]
            Hp = Hp + c
    return Hp


def _batch(P, rows, seed):
    return np.random.default_rng(seed).standard_normal((P + 1, rows))


@pytest.mark.parametrize("P", PARAMS)
def test_hook_new_form_against_parent_and_numpy(forms, P):
    """nt = 1, 2, 3; a full and a one-column last tile; one block, a one-row last block, block counts 1 .. 4"""
    on, off = forms
    for rows in ROWS:
        E = _batch(P, rows, 1000 * P + rows)
        for formed in (False, True):
            h = 1e-3 if not formed else 1.0
            new, old = on.normalEquationsOf(E, h, formed), off.normalEquationsOf(E, h, formed)
            _same_bits(new, old, (P, rows, formed))
            _same_bits(new, new.T, (P, rows, formed, "mirror"))
            _same_bits(new, _numpy_normal_equations(E, h, formed), (P, rows, formed, "numpy"))


SPECIAL = {"nan": np.nan, "inf": np.inf, "minus_zero": -0.0, "denormal": 5e-324 * 12345}


@pytest.mark.parametrize("name", sorted(SPECIAL))
@pytest.mark.parametrize("where", ["e0", "column"])
def test_hook_special_values(forms, name, where):
    on, off = forms
    for P, rows in ((30, 513), (33, 257), (64, 769)):
        E = _batch(P, rows, 7 * P + rows)
        E[0 if where == "e0" else min(P, 34), rows - 2] = SPECIAL[name]
        if name == "minus_zero":  # a whole column of -0.0 as well: products of either sign of zero
            E[1 if where == "e0" else 2] = -0.0
        for formed in (False, True):
            new, old = on.normalEquationsOf(E, 0.5, formed), off.normalEquationsOf(E, 0.5, formed)
            _same_bits(new, old, (name, where, P, rows, formed))
            _same_as_numpy(new, _numpy_normal_equations(E, 0.5, formed), (name, where, P, rows, formed))
            if name in ("nan", "inf"):
                assert np.isnan(new).any() or np.isinf(new).any()


# ---- whole calls: switch 1 against 0 on fresh contexts ----
def _optimize(hip, problems, debug, fixed_iters=True, contexts=1, **ctx_args):
    """optimizeSet problem after problem (problem i on context i % contexts) -> per problem (poses, global points, report, trace)"""
    opts = [hip.DmsaOptimizer(fixed_iters=fixed_iters, debug=debug, **ctx_args) for _ in range(contexts)]
    out = []
    for i, (prob, s) in enumerate(problems):
        opt, p = opts[i % contexts], prob.copy()
        r = opt.optimizeSet(p, s)
        rep = (r.iterations, r.stop_reason, r.evaluations, r.num_gaussians, r.num_gaussians_l1, r.num_memberships, r.error0, r.last_step_norm, r.last_line_search_k)
        tr = [(t["M"], t["M1"], t["Mm"], t["best_k"], t["error0"], t["step_norm"]) for t in opt.trace()[: r.iterations]]
        out.append((p.relOrientations.copy(), p.relTranslations.copy(), opt.globalPoints(), rep, tr))
    for opt in opts:
        assert opt.debugCounters()["sync_retries"] == 0
        opt.close()
    return out


def _same_runs(a, b):
    assert len(a) == len(b)
    for (oa, ta, ga, ra, tra), (ob, tb, gb, rb, trb) in zip(a, b):
        assert np.array_equal(_bits(np.array(ra[6:8])), _bits(np.array(rb[6:8]))) and ra[:6] == rb[:6] and ra[8] == rb[8]
        assert len(tra) == len(trb)
        for x, y in zip(tra, trb):
            assert x[:4] == y[:4] and np.array_equal(_bits(np.array(x[4:])), _bits(np.array(y[4:])))
        for x, y in ((oa, ob), (ta, tb)):
            assert np.array_equal(_bits(x), _bits(y))
        assert np.array_equal(np.ascontiguousarray(ga).view(np.uint8), np.ascontiguousarray(gb).view(np.uint8))


def _on_off(hip, problems, **kw):
    off = _optimize(hip, problems, OFF, **kw)
    _same_runs(_optimize(hip, problems, ON, **kw), off)
    return off


def _window(**kw):
    """the suite's small window: 8 144 points, P = 30"""
    return synth.window_problem(seed=1, scans=3, rings=16, az_steps=128, num_static=2000, **kw)


def _one_block():
    return synth.window_problem(seed=5, scans=3, rings=8, az_steps=36, num_static=100, grid_size=1.0)


def test_small_window(hip):
    s = DmsaOptimSettings.sliding_window(num_iter=6)
    off = _on_off(hip, [(_window(), s)])
    assert off[0][3][0] == 6
    _same_runs(_optimize(hip, [(_window(), s)], None), off)  # the default is the new form


@pytest.mark.parametrize("poses", [7, 11])
def test_window_with_two_tiles(hip, poses):
    """P = 36 and 60: nt = 2, three tile pairs, one of them off the diagonal"""
    off = _on_off(hip, [(_window(num_control_poses=poses), DmsaOptimSettings.sliding_window(num_iter=3))])
    assert off[0][3][0] == 3


def test_imu_window(hip):
    """additional rows behind the Gaussians'"""
    prob = synth.window_problem(seed=5, scans=4, rings=16, az_steps=96, num_static=3000, use_imu=True)
    off = _on_off(hip, [(prob, DmsaOptimSettings.sliding_window(use_imu=True, num_iter=4))])
    assert off[0][3][0] == 4


def test_analytic_jacobian_window(hip):
    """formed columns (kFormed) inside a whole call"""
    s = DmsaOptimSettings.sliding_window(num_iter=3)
    s.use_analytic_jacobi = True
    off = _on_off(hip, [(_window(), s)])
    assert off[0][3][0] == 3


def test_keyframe_set_up_to_60_parameters(hip):
    prob = synth.keyframe_problem(seed=5, frames=8, rings=24, az_steps=160, arc=0.5)  # P = 42
    off = _on_off(hip, [(prob, DmsaOptimSettings.keyframe_map(num_iter=2))])
    assert off[0][3][0] == 2


def test_keyframe_neighbourhood_keeps_the_parents_launches(hip):
    """P = 186: matrix-core normal equations with either value"""
    prob = synth.keyframe_problem(seed=9, frames=32, rings=16, az_steps=128, arc=1.2)
    off = _on_off(hip, [(prob, DmsaOptimSettings.keyframe_map(num_iter=2))])
    assert off[0][3][0] == 2


def test_three_calls_of_two_sizes_and_two_contexts(hip):
    """other row counts on one context (the block sums of a larger call stay behind in the buffer), and two contexts used alternately"""
    s = DmsaOptimSettings.sliding_window(num_iter=3)
    calls = [(_one_block(), s), (_window(), s), (_one_block(), s)]
    off = _on_off(hip, calls)
    _same_runs(off[2:], off[:1])
    _same_runs(_optimize(hip, calls + calls[1:2], ON, contexts=2), off + off[1:2])


def test_early_exit(hip):
    """NO_IMPROVEMENT in the eighth iteration, and a second call on the same context behind it"""
    s = DmsaOptimSettings.sliding_window(num_iter=10)
    off = _on_off(hip, [(_window(), s), (_window(), s)], fixed_iters=False)
    assert off[0][3][:2] == (8, STOP_NO_IMPROVEMENT), off[0][3]


def test_event_dependencies_host_loop_and_stage_timers(hip, monkeypatch):
    s = DmsaOptimSettings.sliding_window(num_iter=3)
    off = _optimize(hip, [(_window(), s)], OFF)
    _same_runs(_optimize(hip, [(_window(), s)], ON, stage_timers=True), off)
    _same_runs(_optimize(hip, [(_window(), s)], dict(ON, device_loop=0)), _optimize(hip, [(_window(), s)], dict(OFF, device_loop=0)))
    monkeypatch.setenv("DMSA_DEBUG", "device_sync=0")
    _same_runs(_optimize(hip, [(_window(), s)], ON), off)


def test_stage_call(hip):
    """dmsa_normal_equations on a resident window (Gaussian rows alone, default and explicit switch), against the hook on the same batch"""
    h, lam = float(np.sqrt(np.finfo(np.float32).eps)), 0.0
    prob, s = _window(), DmsaOptimSettings.sliding_window()
    got = []
    for debug in (ON, OFF, None):
        opt = hip.DmsaOptimizer(debug=debug)
        opt.upload(prob)
        base = prob.getPoseParameters()
        opt.poseTables(base, download=False)
        opt.updateGlobalPoints(0, download=False)
        opt.buildGaussians(s)
        P = len(base)
        opt.poseTables(np.concatenate([base[None], base[None] + h * np.eye(P)]), download=False)
        E = opt.evalResiduals(P + 1)
        H, g = opt.normalEquations(P, h, lam, None)
        Hp = opt.normalEquationsOf(E, h)
        _same_bits(H, Hp[:P, :P], debug)
        _same_bits(g, Hp[:P, P], debug)
        got.append((E, H, g))
        opt.close()
    for E, H, g in got[1:]:
        _same_bits(E, got[0][0], "residuals")
        _same_bits(H, got[0][1], "H")
        _same_bits(g, got[0][2], "g")
