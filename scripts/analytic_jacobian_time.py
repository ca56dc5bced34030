"""analytic_jacobian_time.py — optimizeSet with the numeric Jacobian (use_analytic_jacobi = 0, the parity path) and the analytic one
(use_analytic_jacobi = 1) timed in the same process, alternating, after warm-up, on four shapes:

  bench window          10 x 131 072 points + 200 000 static, P = 30
  everyday window       5 x 3 000 rosette points + 3 000 static, P = 30
  keyframe neighbourhood 32 keyframes, P = 186
  loop-closure pass     100 keyframes, P = 594 (last_n_keyframes_for_optim: 100)

Each sample is one optimizeResident call of `--iters` iterations with the exits disabled (DMSA_FLAG_FIXED_ITERS), on its own context per
mode; the result is the median over the samples in ms per iteration.  One JSON document goes to stdout (and to --out).

  python scripts/analytic_jacobian_time.py --samples 7 --iters 10 --out profiles/r07_analytic_jacobian_time.json
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dmsa_lidar_slam_amd import synth  # noqa: E402
from dmsa_lidar_slam_amd.api import DmsaOptimizer  # noqa: E402
from dmsa_lidar_slam_amd.problems import DmsaOptimSettings  # noqa: E402


def shapes(only):
    out = []
    if "bench_window" in only:
        out.append(("bench_window", lambda: synth.window_problem(seed=1), DmsaOptimSettings.sliding_window()))
    if "everyday_window" in only:
        out.append(("everyday_window", lambda: synth.rosette_window_problem(seed=1, scans=5, pts_per_scan=3000, num_static=3000),
                    DmsaOptimSettings.sliding_window()))
    if "keyframes_32" in only:
        out.append(("keyframes_32", lambda: synth.keyframe_problem(seed=5, frames=32, rings=16, az_steps=96, arc=0.07 * 32),
                    DmsaOptimSettings.keyframe_map()))
    if "keyframes_100" in only:
        out.append(("keyframes_100", lambda: synth.keyframe_problem(seed=5, frames=100, rings=16, az_steps=96, arc=0.07 * 100),
                    DmsaOptimSettings.keyframe_map()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", default="bench_window,everyday_window,keyframes_32,keyframes_100")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"iters_per_sample": args.iters, "samples": args.samples, "warmup": args.warmup, "unit": "ms per iteration (median)", "shapes": {}}
    for name, make, base in shapes(args.shapes.split(",")):
        prob = make()
        base = dataclasses.replace(base, num_iter=args.iters)
        runs = {}
        for mode in ("numeric", "analytic"):
            opt = DmsaOptimizer(fixed_iters=True)
            opt.upload(prob.copy())
            runs[mode] = (opt, dataclasses.replace(base, use_analytic_jacobi=mode == "analytic"), [])
        for i in range(args.warmup + args.samples):
            for mode in ("numeric", "analytic"):  # alternating: drift of clocks or temperature hits both modes alike
                opt, s, times = runs[mode]
                t0 = time.perf_counter()
                rep = opt.optimizeResident(s)
                dt = time.perf_counter() - t0
                if i >= args.warmup:
                    times.append(1e3 * dt / max(rep.iterations, 1))
        entry = {"P": prob.numParams, "points": int(prob.localPoints.shape[0])}
        for mode, (opt, s, times) in runs.items():
            entry[mode] = {"ms_per_iter": statistics.median(times), "min": min(times), "max": max(times), "evaluations_per_iter": 10 if mode == "analytic" else prob.numParams + 10}
        entry["speedup"] = entry["numeric"]["ms_per_iter"] / entry["analytic"]["ms_per_iter"]
        result["shapes"][name] = entry
        print(f"[analytic_jacobian_time] {name}: P {entry['P']}: numeric {entry['numeric']['ms_per_iter']:.3f} ms/it, analytic "
              f"{entry['analytic']['ms_per_iter']:.3f} ms/it, x{entry['speedup']:.2f}", file=sys.stderr, flush=True)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
