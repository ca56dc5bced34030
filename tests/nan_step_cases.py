"""Problems and linear systems whose LM step holds a NaN (DmsaOptimizer.h:116-122: setPoseParameters(paramVec); break -> DMSA_STOP_NAN),
for tests/test_nan_step_cases.py (CPU: the oracle's outcome on every one) and tests/test_gpu_nan_step.py (the product against it).

Every named case ends, on the oracle, with iterations = 1, stop_reason = 2, evaluations = 1 + P, last_step_norm = 0, last_line_search_k = 0
and one trace entry (best_k 0, error0 0.0, step_norm 0.0), for num_iter = 1 and 3 alike; the two controls are the same inputs one step away
from the NaN and run all their iterations.  A NaN step in a later iteration of a call cannot be made from inputs: without damping a rank
deficiency shows in iteration 0, with damping there is none.

How the NaN comes about:
  *_last_frame_*    every point of the LAST keyframe is NaN, so no point of it is in a leaf, its six columns of J are zero, and without
                    damping (lambda_diag = 0) the pivot of such a column is 0: 0 / 0
  window_tail       the same with the last 34 % of a window's local points (at 50 % the call stops with too few Gaussians instead)
  *_measurement     a NaN measurement in an additional row: e0 itself, and with it report.error0, is NaN
  window_alpha_* / window_lambda_nan   non-finite settings on an ordinary window; error0 stays finite"""
import functools

import numpy as np
from scipy.spatial.transform import Rotation as Rot

from dmsa_lidar_slam_amd import synth
from dmsa_lidar_slam_amd.problems import DmsaOptimSettings

STOP_NAN = 2  # include/dmsa_hip.h: dmsa_stop_reason

# name -> (frames, seed, rings, az_steps, arc): P = 6 (frames - 1) reaches k_loop_lm_step (30), the stream or the panels (72), the panels
# (198) and the host solve behind the device loop (1194, the shape of test_a_keyframe_set_whose_chain_state_outgrows_64_kb_of_lds)
KEYFRAME_SHAPES = {
    "keyframes_last_frame_P30": (6, 5, 24, 160, 0.4),
    "keyframes_last_frame_P72": (13, 4, 16, 96, 0.8),
    "keyframes_last_frame_P198": (34, 4, 16, 96, 0.8),
    "keyframes_last_frame_P1194": (200, 8, 8, 48, 5.5),
}
WINDOW_CASES = ("window_tail", "window_imu_measurement", "window_alpha_nan", "window_alpha_inf", "window_lambda_nan")
NAN_CASES = tuple(KEYFRAME_SHAPES) + ("keyframes_odometry_measurement",) + WINDOW_CASES
CONTROLS = ("control_damped", "control_middle_frame")  # keyframes_last_frame_P30 with lambda_diag = 1e-5 / with a middle frame emptied
ERROR0_IS_NAN = ("keyframes_odometry_measurement", "window_imu_measurement")
ORACLE_NEEDS_MINUTES = ("keyframes_last_frame_P1194",)


def keyframes(name):
    frames, seed, rings, az_steps, arc = KEYFRAME_SHAPES[name]
    return synth.keyframe_problem(seed=seed, frames=frames, rings=rings, az_steps=az_steps, arc=arc)


def empty_frame(prob, frame):
    """every point of `frame` NaN (xyz; w stays 1)"""
    a, b = int(prob.frameOffsets[frame]), int(prob.frameOffsets[frame + 1])
    prob.localPoints[a:b, :3] = np.nan
    return prob


def small_window():
    """864 local points and 100 static ones, P = 30"""
    return synth.window_problem(seed=5, scans=3, rings=8, az_steps=36, num_static=100, grid_size=1.0)


def odometry_keyframes():
    """the keyframes_gravity_odometry construction of tests/test_gpu_loop.py::_cases"""
    kf = synth.keyframe_problem(seed=5, frames=6, rings=24, az_steps=160, arc=0.4)
    rng = np.random.default_rng(0)
    ro, rt = kf.truth_relative
    kf.useOdometryErrorTerms = True
    kf.odomRelTransl = rt + rng.normal(0, 0.005, rt.shape)
    kf.odomRelOrientMat = (Rot.from_rotvec(ro) * Rot.from_rotvec(rng.normal(0, 1e-3, (kf.numFrames, 3)))).as_matrix()
    kf.__post_init__()
    return kf


def is_window(name):
    return name in WINDOW_CASES


def build(name, num_iter=3):
    """-> (problem, settings); optimize a copy of the problem"""
    kf_s = DmsaOptimSettings.keyframe_map(num_iter=num_iter)
    win_s = DmsaOptimSettings.sliding_window(num_iter=num_iter)
    if name in KEYFRAME_SHAPES:
        prob = keyframes(name)
        kf_s.lambda_diag = 0.0
        return empty_frame(prob, prob.numFrames - 1), kf_s
    if name == "control_damped":  # (lambda_diag stays at the reference's 1e-5)
        prob = keyframes("keyframes_last_frame_P30")
        return empty_frame(prob, prob.numFrames - 1), kf_s
    if name == "control_middle_frame":  # later frames hang on the emptied frame's parameters: no zero column
        prob = keyframes("keyframes_last_frame_P30")
        kf_s.lambda_diag = 0.0
        return empty_frame(prob, prob.numFrames // 2), kf_s
    if name == "keyframes_odometry_measurement":
        prob = odometry_keyframes()
        prob.odomRelTransl[2, 0] = np.nan
        return prob, kf_s
    if name == "window_tail":
        prob = small_window()
        n = prob.localPoints.shape[0]
        prob.localPoints[n - (34 * n) // 100:, :3] = np.nan
        win_s.lambda_diag = 0.0
        return prob, win_s
    if name == "window_imu_measurement":
        prob = synth.window_problem(seed=7, scans=5, rings=16, az_steps=64, num_static=300, use_imu=True)
        prob.preintRelPositions[1, 0] = np.nan
        return prob, DmsaOptimSettings.sliding_window(use_imu=True, num_iter=num_iter)
    if name == "window_alpha_nan":
        win_s.step_length_optim = float("nan")
    elif name == "window_alpha_inf":
        win_s.step_length_optim = float("inf")
    elif name == "window_lambda_nan":
        win_s.lambda_diag = float("nan")
    else:
        raise KeyError(name)
    return small_window(), win_s


def ordinary(name):
    """an ordinary problem of the model of NaN case `name` (part C: the calls around the NaN call) -> (problem, another problem)"""
    if is_window(name):
        return small_window(), synth.window_problem(seed=3, scans=3, rings=16, az_steps=48, num_static=150, grid_size=1.0)  # (2 304 points: three blocks)
    return keyframes("keyframes_last_frame_P72"), synth.keyframe_problem(seed=6, frames=9, rings=16, az_steps=96, arc=0.6)


# ---- the solve alone ---------------------------------------------------------------------------------------------------------------
KINDS = ("zero_column", "equal_columns", "nan_entry")


def singular_system(orc, P, kind, cols, seed):
    """H = J^T J (no damping), g = J^T e0 for a random J of (4 P + 5) x P that `kind` spoils at the columns `cols`, and the set of positions
    at which the oracle's step (alpha = 0.2) is NaN -> (H_damped, g, nan_positions).
    zero_column: J[:, c] = 0 for every c of cols (the pivot of c is 0: 0 / 0 in row c, and nowhere else); equal_columns: J[:, c] = J[:, 0]
    for every c of cols; nan_entry: J[r, c] = nan for one row r."""
    rng = np.random.default_rng(seed)
    rows = 4 * P + 5
    J = rng.normal(size=(rows, P))
    e0 = rng.uniform(0.5, 2.0, rows)
    for c in cols:
        if kind == "zero_column":
            J[:, c] = 0.0
        elif kind == "equal_columns":
            assert c != 0
            J[:, c] = J[:, 0]
        elif kind == "nan_entry":
            J[int(rng.integers(rows)), c] = np.nan
        else:
            raise KeyError(kind)
    H, g, step = orc.lm_step_from_jacobian(e0, J, 0.0, 0.2)
    return H, g, frozenset(int(i) for i in np.flatnonzero(np.isnan(step)))


def boundary_columns(P):
    """0, 1, P - 2, P - 1 and the columns on each side of every multiple of 64 below P"""
    return sorted({c for c in (0, 1, 63, 64, 65, 127, 128, 129, P - 2, P - 1) if 0 <= c < P})


def solve_columns(P):
    """the zero columns tried at P: the largest size keeps 0, P - 1 and the first 64-boundary (a system of it takes the oracle seconds)"""
    return [0, 63, 64, P - 1] if P == 594 else boundary_columns(P)


# P -> lm_stream values: k_loop_lm_step (<1,4> up to 16 = 4 kSolveWaves, <2,kSolveRows> beyond), the stream and the panels on the same
# sizes, the panels alone beyond 192
SOLVE_TIERS = {6: (1,), 16: (1,), 17: (1,), 30: (1,), 64: (1,), 65: (1, 0), 128: (1, 0), 129: (1, 0), 186: (1, 0), 192: (1, 0), 193: (1,), 594: (1,)}
ONE_PER_TIER = ((30, 1), (129, 1), (129, 0), (193, 1))  # (P, lm_stream) for equal_columns and nan_entry


@functools.lru_cache(maxsize=None)
def regular_system(orc, P):
    """the well-posed system of tests/test_gpu_loop.py::_system(orc, P, 300 + P): forward differences, two exactly dependent columns under
    the reference's weak damping -> (H_damped, g, the oracle's step).  Diagonally dominant: the solve makes no row swap and meets no tie on
    it (tests/test_lm_pivot_cases.py asserts that; tests/lm_pivot_cases.py holds the systems that do)"""
    rng = np.random.default_rng(300 + P)
    rows = 4 * P + 50
    e0 = rng.uniform(0.5, 2.0, rows)
    eb = e0[None, :] + rng.normal(size=(P, rows)) * 1e-4
    eb[P // 3] = eb[P // 3 + 1]
    h = float(np.sqrt(np.finfo(np.float32).eps))
    H, g, step = orc.lm_step(e0, eb, h, float(np.float32(1e-5)), 0.2)
    return H.reshape(P, P), g, step


# ---- comparing runs ------------------------------------------------------------------------------------------------------------------
REPORT_INTS = ("iterations", "stop_reason", "evaluations", "num_gaussians", "num_gaussians_l1", "num_memberships", "last_line_search_k")
REPORT_FLOATS = ("error0", "last_step_norm")


def bits(x):
    return int(np.float64(x).view(np.uint64))


def run_record(prob_after, rep, trace, global_points=None):
    """what same_run compares: the poses, the report, the trace of the iterations that ran and (optionally) the global points"""
    return dict(orient=prob_after.relOrientations.copy(), transl=prob_after.relTranslations.copy(), points=global_points,
                ints=tuple(int(getattr(rep, k)) for k in REPORT_INTS), floats=tuple(float(getattr(rep, k)) for k in REPORT_FLOATS),
                trace=[(t["M"], t["M1"], t["Mm"], t["best_k"], float(t["error0"]), float(t["step_norm"])) for t in trace[: rep.iterations]])


def same_run(a, b):
    """Every integer equal, every float of report, trace and poses the same BITS: error0 is NaN where a measurement is, and NaN != NaN would
    fail a correct run, while a comparison that forgives NaNs would pass one NaN for another number's place.  The global points are float32
    and compared by bits as well, except where BOTH sides hold a NaN: those are the emptied points themselves, and which NaN an arithmetic
    operation returns for a NaN operand is the processor's choice (IEEE 754-2008, 6.2.3)."""
    assert a["ints"] == b["ints"], (a["ints"], b["ints"])
    assert [bits(x) for x in a["floats"]] == [bits(x) for x in b["floats"]], ([hex(bits(x)) for x in a["floats"]], [hex(bits(x)) for x in b["floats"]])
    assert len(a["trace"]) == len(b["trace"])
    for ta, tb in zip(a["trace"], b["trace"]):
        assert ta[:4] == tb[:4] and [bits(x) for x in ta[4:]] == [bits(x) for x in tb[4:]], (ta, tb)
    for k in ("orient", "transl"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (k, np.abs(a[k] - b[k]).max())
    if a["points"] is not None and b["points"] is not None:
        pa, pb = np.ascontiguousarray(a["points"], np.float32), np.ascontiguousarray(b["points"], np.float32)
        assert pa.shape == pb.shape
        same = (pa.view(np.uint32) == pb.view(np.uint32)) | (np.isnan(pa) & np.isnan(pb))
        assert same.all(), np.argwhere(~same)[:5]


def literal_nan_stop(rec, P, evaluations=None):
    """the outcome spelled out, so that a mistake both sides of same_run share cannot pass"""
    it, stop, evals = rec["ints"][0], rec["ints"][1], rec["ints"][2]
    assert (it, stop, evals) == (1, STOP_NAN, 1 + P if evaluations is None else evaluations), rec["ints"]
    assert rec["ints"][6] == 0 and bits(rec["floats"][1]) == 0, (rec["ints"], rec["floats"])
    assert len(rec["trace"]) == 1 and rec["trace"][0][3] == 0 and bits(rec["trace"][0][4]) == 0 and bits(rec["trace"][0][5]) == 0, rec["trace"]
