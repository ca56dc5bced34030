#!/usr/bin/env python
"""Does a build of the library enqueue the kernels of whole optimizeSet calls in the order another build does?  (csrc/optimize_loop.cpp: the
iteration rate rests on the order of the host's launches, per stream and across streams.)

    rocprofv3 --kernel-trace -d DIR_A -o trace -- python scripts/loop_driver_order.py run        # with DMSA_LIB_PATH at build A
    rocprofv3 --kernel-trace -d DIR_B -o trace -- python scripts/loop_driver_order.py run        # ... at build B
    python scripts/loop_driver_order.py compare A_results.db B_results.db > profiles/rNN_loop_driver_order.txt

`run` drives three small fixed-seed problems (the IMU window, the plain window and the P = 72 keyframe set of tests/test_gpu_loop.py) for three
iterations through one context per mode the loop's plan decides (CONTEXTS); a small torch kernel in front of each context marks where its
kernels begin in the trace.  `compare` cuts the two rocpd databases at those marks and compares, context by context, the sequence of (kernel
name, grid size) per hardware queue and per stream: "identical" or the first difference.  Kernel times and the interleaving of the queues
are not compared: they vary from run to run.  A context that fell back to event dependencies under the tracer says so in its line of `run`."""
import os
import sqlite3
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, problem, debug, constructor flags, settings)
CONTEXTS = [
    ("window_imu defaults", "imu", {}, {}, {}),
    ("window_imu device_sync=0", "imu", {"device_sync": 0}, {}, {}),
    ("window_imu dual_stream=0", "imu", {"dual_stream": 0}, {}, {}),
    ("window_imu serial_streams=1", "imu", {"serial_streams": 1}, {}, {}),
    ("window_imu serial_streams=2", "imu", {"serial_streams": 2}, {}, {}),
    ("window_imu trial_rows_aside=0", "imu", {"trial_rows_aside": 0}, {}, {}),
    ("window_imu gap_stamps=2", "imu", {"gap_stamps": 2}, {}, {}),
    ("window_imu one_readback=0 batch_stamps=0", "imu", {"one_readback": 0, "batch_stamps": 0}, {}, {}),
    ("window_imu next_head=3", "imu", {"next_head": 3}, {}, {}),
    ("window_imu long_split=2 device_sync=0", "imu", {"long_split": 2, "device_sync": 0}, {}, {}),
    ("window_imu analytic", "imu", {}, {}, {"use_analytic_jacobi": True}),
    ("window_imu STAGE_TIMERS", "imu", {}, {"stage_timers": True}, {}),
    ("window_plain defaults", "plain", {}, {}, {}),
    ("window_plain next_head=0", "plain", {"next_head": 0}, {}, {}),
    ("keyframes_P72 defaults", "kf", {}, {}, {}),
    ("keyframes_P72 eval_skip=2 lm_stream=0", "kf", {"eval_skip": 2, "lm_stream": 0}, {}, {}),
    ("keyframes_P72 device_loop=0", "kf", {"device_loop": 0}, {}, {}),
]


def run():
    import torch

    from dmsa_lidar_slam_amd import synth
    from dmsa_lidar_slam_amd.api import DmsaOptimizer
    from dmsa_lidar_slam_amd.problems import DmsaOptimSettings

    problems = {"imu": (synth.window_problem(seed=7, scans=5, rings=16, az_steps=256, num_static=1500, use_imu=True), lambda: DmsaOptimSettings.sliding_window(use_imu=True, num_iter=3)),
                "plain": (synth.window_problem(seed=31, scans=3, rings=32, az_steps=256, num_static=4000), lambda: DmsaOptimSettings.sliding_window(num_iter=3)),
                "kf": (synth.keyframe_problem(seed=4, frames=13, rings=16, az_steps=96, arc=0.8), lambda: DmsaOptimSettings.keyframe_map(num_iter=3))}
    for i, (name, which, debug, ctor, sset) in enumerate(CONTEXTS):
        torch.zeros(256 * (i + 1), device="cuda")  # the mark
        torch.cuda.synchronize()
        prob, mk = problems[which]
        s = mk()
        for k, v in sset.items():
            setattr(s, k, v)
        opt = DmsaOptimizer(device=0, debug=debug or None, **ctor)
        p = prob.copy()
        rep = opt.optimizeSet(p, s)
        print(f"[{i}] {name}: {rep.iterations} iterations, {rep.num_gaussians} Gaussians, sync_retries {opt.debugCounters()['sync_retries']}, lastError {opt.lastError()!r}", flush=True)
        opt.close()
        torch.cuda.synchronize()


def short(name):
    return name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("dmsa::", "")


def contexts_of(path):
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    grid = [c for c in cols if c.startswith("grid")]
    qcol = "queue_id" if "queue_id" in cols else "stream_id"
    rows = db.execute(f"select name, {qcol}, stream_id, {', '.join(grid)} from kernels order by start").fetchall()
    out = []
    for name, queue, stream, *g in rows:
        if "at::native" in name:
            out.append(({}, {}))
        elif out:
            out[-1][0].setdefault(queue, []).append((short(name), tuple(g)))
            out[-1][1].setdefault(stream, []).append((short(name), tuple(g)))
    return [([c[0][q] for q in sorted(c[0])], [c[1][q] for q in sorted(c[1])]) for c in out]


def compare(path_a, path_b):
    a, b = contexts_of(path_a), contexts_of(path_b)
    print(f"# per-queue and per-stream sequences of (kernel name, grid) under rocprofv3 --kernel-trace: A = {path_a}, B = {path_b}; {len(a)} / {len(b)} contexts")
    same = len(a) == len(b) == len(CONTEXTS)
    for i, (ca, cb) in enumerate(zip(a, b)):
        verdict = []
        for kind, xa, xb in (("queue", ca[0], cb[0]), ("stream", ca[1], cb[1])):
            what = None
            if len(xa) != len(xb):
                what = f"{len(xa)} {kind}s in A, {len(xb)} in B"
            else:
                for q, (sa, sb) in enumerate(zip(xa, xb)):
                    if sa != sb:
                        k = next((k for k, (x, y) in enumerate(zip(sa, sb)) if x != y), min(len(sa), len(sb)))
                        what = f"{kind} {q}, kernel {k} of {len(sa)}/{len(sb)}: A {sa[k] if k < len(sa) else None}, B {sb[k] if k < len(sb) else None}"
                        break
            same = same and not what
            verdict.append(f"{kind}s {'DIFFERENT at ' + what if what else 'identical'} ({sum(map(len, xa))} kernels on {len(xa)})")
        print(f"[{i}] {CONTEXTS[i][0]}: " + "; ".join(verdict))
    print("identical" if same else "DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run()
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
