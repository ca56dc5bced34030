#!/usr/bin/env python
"""Does a build of the library enqueue the voxelisation's kernels in the order another build does?  (csrc/voxelize_driver.cpp: the order of the
host's launches alone moves the headline by 14 %.)

    rocprofv3 --kernel-trace -d DIR_A -o trace -- python scripts/voxel_driver_order.py run        # with DMSA_LIB_PATH at build A
    rocprofv3 --kernel-trace -d DIR_B -o trace -- python scripts/voxel_driver_order.py run        # ... at build B
    python scripts/voxel_driver_order.py compare A_results.db B_results.db > profiles/rNN_voxel_driver_order.txt

`run` drives fixed-seed problems for a fixed number of iterations through one context per mode of build_gaussians (CONTEXTS); a small torch
kernel in front of each context marks where its kernels begin in the trace.  `compare` cuts the two rocpd databases at those marks and
compares, context by context and stream by stream, the sequence of (kernel name, grid size): "identical" or the first difference.
The timing of the kernels and the interleaving of the streams are not compared: they vary from run to run."""
import os
import sqlite3
import sys

# (name, problem, debug switches, resident calls behind the one upload, iterations per call)
CONTEXTS = [
    ("default window, past the streak of eight", "window", {}, 4, 6),
    ("keys_ahead=2", "window", {"keys_ahead": 2}, 1, 5),
    ("keys_ahead=0", "window", {"keys_ahead": 0}, 1, 5),
    ("fit_by_level=0", "window", {"fit_by_level": 0}, 1, 5),
    ("fit_by_level=2, small window", "mid", {"fit_by_level": 2}, 1, 5),
    ("merge_sort=1", "window", {"merge_sort": 1}, 1, 5),
    ("small_voxel=1, 29 576 points", "small", {"small_voxel": 1}, 1, 5),
    ("dual_stream=0", "window", {"dual_stream": 0}, 1, 5),
    ("device_sync=0", "window", {"device_sync": 0}, 1, 5),
    ("speculation_fault=2", "window", {"speculation_fault": 2}, 1, 5),
    ("keyframes, gauss_split", "keyframes", {}, 1, 3),
]


def run():
    import torch

    from dmsa_lidar_slam_amd import synth
    from dmsa_lidar_slam_amd.api import DmsaOptimizer
    from dmsa_lidar_slam_amd.problems import DmsaOptimSettings

    problems = {
        "window": synth.window_problem(seed=1),  # the bench window: 1.5 M points, a sort per level
        "mid": synth.window_problem(seed=2, scans=5, rings=32, az_steps=512, num_static=10_000),
        "small": synth.window_problem(seed=3, scans=3, rings=32, az_steps=256, num_static=5_000),
        "keyframes": synth.keyframe_problem(seed=1, frames=8),
    }
    for i, (name, which, debug, calls, iters) in enumerate(CONTEXTS):
        torch.zeros(256 * (i + 1), device="cuda")  # the mark
        torch.cuda.synchronize()
        settings = DmsaOptimSettings.keyframe_map(num_iter=iters) if which == "keyframes" else DmsaOptimSettings.sliding_window(num_iter=iters)
        opt = DmsaOptimizer(device=0, fixed_iters=True, debug=debug or None)
        opt.upload(problems[which])
        for _ in range(calls):
            rep = opt.optimizeResident(settings)
        print(f"[{i}] {name}: {rep.iterations} iterations, {rep.num_gaussians} Gaussians, counters {opt.debugCounters()}", flush=True)
        opt.close()
        torch.cuda.synchronize()


def is_mark(name):
    return "at::native" in name


def short(name):
    return name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("dmsa::", "")


def contexts_of(path):
    """-> per context, per stream in the order of the stream ids (the order the context created them in): [(kernel, grid)]"""
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    grid = [c for c in cols if c.startswith("grid")]
    rows = db.execute(f"select name, stream_id, {', '.join(grid)} from kernels order by start").fetchall()
    out = []
    for name, stream, *g in rows:
        if is_mark(name):
            out.append({})
        elif out:
            out[-1].setdefault(stream, []).append((short(name), tuple(g)))
    return [[c[stream] for stream in sorted(c)] for c in out]


def compare(path_a, path_b):
    a, b = contexts_of(path_a), contexts_of(path_b)
    print(f"# per-stream sequences of (kernel name, grid size) of `scripts/voxel_driver_order.py run` under rocprofv3 --kernel-trace: A = {path_a}, B = {path_b}")
    same = len(a) == len(b) == len(CONTEXTS)
    if not same:
        print(f"DIFFERENT: {len(a)} contexts in A, {len(b)} in B, {len(CONTEXTS)} expected")
    for i, (ca, cb) in enumerate(zip(a, b)):
        name = CONTEXTS[i][0] if i < len(CONTEXTS) else "?"
        what = None
        if len(ca) != len(cb):
            what = f"{len(ca)} streams in A, {len(cb)} in B"
        for s, (sa, sb) in enumerate(zip(ca, cb)):
            if what:
                break
            for k, (x, y) in enumerate(zip(sa, sb)):
                if x != y:
                    what = f"stream {s}, kernel {k}: A {x}, B {y}"
                    break
            if not what and len(sa) != len(sb):
                what = f"stream {s}: {len(sa)} kernels in A, {len(sb)} in B (equal up to the shorter)"
        same = same and not what
        print(f"[{i}] {name}: {'DIFFERENT at ' + what if what else 'identical'}  ({sum(map(len, ca))} kernels on {len(ca)} streams)")
    print("identical" if same else "DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        run()
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
