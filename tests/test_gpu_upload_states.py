"""The state rule of an upload (csrc/upload_driver.cpp): a refusal by an entry's argument checks leaves the resident problem exactly as it
was; a failure between upload_begin and upload_commit leaves NO resident problem -- every call that needs one is refused instead of running
on buffers of two problems --; a later valid upload works as on a fresh context.  And the contract of the pinned staging area (StageArea,
csrc/dmsa_ctx.h) and of dmsa_reserve beside a resident problem."""
import ctypes as C

import numpy as np
import pytest

from dmsa_lidar_slam_amd import _capi as capi
from dmsa_lidar_slam_amd import synth
from dmsa_lidar_slam_amd.problems import DmsaOptimSettings

pytestmark = pytest.mark.gpu

S_W = DmsaOptimSettings.sliding_window(num_iter=1)
S_K = DmsaOptimSettings.keyframe_map(num_iter=1)


def _window(seed=38, **kw):
    return synth.window_problem(seed=seed, **{**dict(scans=2, rings=8, az_steps=64, num_static=100), **kw})


def _keyframes(seed=41):
    return synth.keyframe_problem(seed=seed, frames=3, rings=8, az_steps=64, arc=0.1)


def _settings(p):
    return S_W if hasattr(p, "trajTime") else S_K


def _run(opt, s):
    """optimizeResident -> everything a caller sees of it: poses, report fields, trace."""
    rep = opt.optimizeResident(s)
    ro, rt = opt.poses()
    fields = (rep.iterations, rep.stop_reason, rep.num_gaussians, rep.num_memberships, rep.evaluations, rep.error0)
    trace = [(t["M"], t["M1"], t["Mm"], t["best_k"], t["error0"], t["step_norm"]) for t in opt.trace()[: rep.iterations]]
    return np.concatenate([ro.ravel(), rt.ravel()]), fields, trace


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]


def _fresh(hip, p):
    o = hip.DmsaOptimizer()
    o.upload(p.copy())
    out = _run(o, _settings(p))
    o.close()
    return out


def _bad_tform(p):
    bad = p.copy()
    bad.tformIdPerPoint = bad.tformIdPerPoint.copy()
    bad.tformIdPerPoint[5] = bad.trajTime.shape[0]  # == n_total: one past the last row
    return bad


def _coincident_stamps(p):
    bad = p.copy()
    bad.stamps = bad.stamps.copy()
    bad.stamps[2] = bad.stamps[1]
    return bad


def _fill_ring(opt, p):
    off = p.scanOffsets
    opt.ringCreate(len(off) - 1, int(np.diff(off).max()), p.staticPoints.shape[0], p.trajTime.size, p.relOrientations.shape[0])
    for k in range(len(off) - 1):
        opt.ringPushAos(p.localPoints[off[k]:off[k + 1]], p.pointStamps[off[k]:off[k + 1]], p.ringIds[off[k]:off[k + 1]])


def _assert_no_resident_problem(hip, opt, s):
    for call in (lambda: opt.optimizeResident(s), lambda: opt.evalResiduals(1, download=False), opt.poses, opt.globalPoints):
        with pytest.raises(hip.DmsaError):
            call()


def test_refused_after_begin_leaves_no_resident_problem(hip):
    p = _window()
    opt = hip.DmsaOptimizer()
    _fill_ring(opt, p)
    two_poses = _window(seed=39, num_control_poses=2)
    attempts = [("tform_idx", lambda: opt.upload(_bad_tform(p))),
                ("tform_idx", lambda: opt.optimizeSetAos(_bad_tform(p), S_W)),
                ("coincident stamps", lambda: opt.upload(_coincident_stamps(p))),
                ("control poses", lambda: opt.uploadFromRing(two_poses, p.t0))]
    for text, attempt in attempts:
        opt.upload(p.copy())
        opt.optimizeResident(S_W)
        with pytest.raises(hip.DmsaError, match=text):
            attempt()
        _assert_no_resident_problem(hip, opt, S_W)
    opt.upload(p.copy())
    assert _same(_run(opt, S_W), _fresh(hip, p))
    opt.close()


def test_refused_before_begin_leaves_the_resident_problem_intact(hip):
    p = _window()
    opt, twin = hip.DmsaOptimizer(), hip.DmsaOptimizer()
    for o in (opt, twin):
        o.upload(p.copy())
        o.optimizeResident(S_W)
    lib, ctx = opt._lib, opt._ctx
    # a null point array with a positive count
    cp = p.to_c()
    cp.xyz_local = None
    with pytest.raises(hip.DmsaError, match="null point arrays"):
        opt._check(lib.dmsa_window_upload(ctx, C.byref(cp)), "upload")
    # frame offsets that decrease
    kf = _keyframes()
    kf.frameOffsets = kf.frameOffsets.copy()
    kf.frameOffsets[1], kf.frameOffsets[2] = kf.frameOffsets[2], kf.frameOffsets[1]
    with pytest.raises(hip.DmsaError, match="frame_offset"):
        opt.upload(kf)
    # a strided view whose stride is no multiple of four
    cloud = np.zeros(p.localPoints.shape[0], hip.DmsaOptimizer.POINT_STAMP_ID)
    idx = np.ascontiguousarray(p.tformIdPerPoint, np.int32)
    views = (capi.AosView * 1)()
    views[0] = opt._view(cloud, 24, idx)
    views[0].stride = 30
    with pytest.raises(hip.DmsaError, match="invalid window cloud view"):
        opt._check(lib.dmsa_window_upload_aos(ctx, C.byref(p.to_c()), views, 1, None), "upload_aos")
    assert _same(_run(opt, S_W), _run(twin, S_W))
    opt.close(), twin.close()


def test_model_switches_with_refused_uploads_between(hip):
    """Extends test_context_reuse_across_sizes_and_models: window, keyframes, larger window, smaller window on one context, a refused upload
    between each pair, each refused after begin: no resident problem in between."""
    small, large = _window(seed=31), _window(seed=32, scans=3, rings=16, az_steps=96, num_static=400)
    probs = [small, _keyframes(seed=33), large, small]
    opt = hip.DmsaOptimizer()
    refusals = [lambda: opt.upload(_bad_tform(small)), lambda: opt.upload(_coincident_stamps(large)), lambda: opt.optimizeSetAos(_bad_tform(large), S_W)]
    got = []
    for k, p in enumerate(probs):
        opt.upload(p.copy())
        got.append(_run(opt, _settings(p)))
        assert _same(got[-1], _fresh(hip, p))
        if k < len(refusals):
            with pytest.raises(hip.DmsaError):
                refusals[k]()
            _assert_no_resident_problem(hip, opt, _settings(p))
    assert _same(got[0], got[3])
    opt.close()


def test_staging_area_is_acquired_behind_the_copy_that_last_read_it(hip):
    """A scan pushed into the ring leaves its copy from the staging area in flight; the AoS upload that follows at once gathers into the
    same area.  The ring's window must come out as the flat upload of that window gives it."""
    a, b = _window(seed=44), _window(seed=45, num_static=300)
    opt = hip.DmsaOptimizer()
    _fill_ring(opt, a)  # the last ringPushAos ...
    opt.optimizeSetAos(b.copy(), S_W)  # ... directly followed by the AoS upload of another window
    opt.uploadFromRing(a.copy(), a.t0)
    assert _same(_run(opt, S_W), _fresh(hip, a))
    opt.close()


@pytest.mark.parametrize("use_imu", [False, True])
def test_reserve_beside_a_resident_problem(hip, use_imu):
    """The reservation moves the problem's arrays, the time grid among them, which the device loop of a window with IMU rows reads through
    the loop model."""
    p = _window(use_imu=use_imu)
    s = DmsaOptimSettings.sliding_window(use_imu=use_imu, num_iter=1)
    opt, twin = hip.DmsaOptimizer(), hip.DmsaOptimizer()
    for o in (opt, twin):
        o.upload(p.copy())
        o.optimizeResident(s)
    n, rows = p.localPoints.shape[0] + p.staticPoints.shape[0], p.trajTime.shape[0]
    before = opt.globalPoints()
    opt._check(opt._lib.dmsa_reserve(opt._ctx, 8 * n, 4 * rows, 60), "reserve")
    assert opt.numTableRows() == rows  # the sizes stay the problem's ...
    assert np.array_equal(opt.globalPoints(), before)  # ... (a capacity of n points still suffices) and so do its points
    assert _same(_run(opt, s), _run(twin, s))
    opt.close(), twin.close()
