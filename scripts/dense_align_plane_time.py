"""Time of the point-to-plane alignment of the dense cloud's reference (include/dmsa_dense_align_plane.h) beside the point-to-point one
(include/dmsa_dense_align.h), on the workload of scripts/dense_align_time.py (profiles/r09_dense_cloud.json: 200 Ouster messages of 131 072
points, voxel 0.1 m; the reference is the store, jittered below half a voxel and moved by the inverse of 0.5 degrees and 0.05 m) and on the
synthetic room of the tests.

    python scripts/dense_align_plane_time.py --out profiles/r23_dense_align_plane.json
    rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- python scripts/dense_align_plane_time.py --kernels-only
    python scripts/dense_align_plane_time.py --trace DIR --out profiles/r23_dense_align_plane.json

The first form times in ONE process, each figure a median of --repeats after a warm-up and each ending in a host wait: compute_normals at
0.3 m (what the plane call needs first), then per max_distance the two stage calls with the grids kept (dmsa_dense_cloud_align_sums and
dmsa_dense_cloud_align_plane_sums: the same search, the sums kernels differ), the two host solves, and both alignment calls end to end with
their time per iteration.  That workload fills a volume (a jittered copy of a voxel-thinned cloud): its normals mean little, so what the
plane call does there is reported and nothing is claimed of its convergence.  The room (dense_align_model.room: 4 920 rows, 2 000 reference
rows, 1 cm noise, 2 degrees and 0.146 m, then 5 degrees and 0.367 m) gives iterations, total time and entry errors of both metrics.
The second form is the device work alone, for a profiler run of its own; the third reads that run's kernel trace: per dispatch of the three
k_align_plane_sums, k_align_pair_sums, k_nearest_across and k_compare_quantise_sum, medians.
No threshold is fixed in advance."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_cloud_time as dct  # noqa: E402  (the sequence generator)
from dense_align_time import rigid  # noqa: E402
from dense_normals_time import spread, timed  # noqa: E402

REACHES = (0.3, 1.0)
KERNELS = ("LinearWords", "SquareWords", "ResidualWords", "k_align_pair_sums", "k_nearest_across", "k_compare_quantise_sum")


def trace_figures(directory):
    """Durations [ms] per dispatch from the *kernel_trace.csv of a rocprofv3 --kernel-trace run."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6) for r in csv.DictReader(open(path))]
    out = {}
    for name in KERNELS:
        ms = [t for kernel, t in rows if name in kernel]
        if ms:
            key = name if name.startswith("k_") else f"k_align_plane_sums<{name}>"
            out[key + "_ms"] = {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "dispatches": len(ms)}
    return out


def both_metrics(dc, ref, reach, repeats, motion, iterations=30):
    """Both alignment calls end to end on the object as it stands (normals computed): per metric the call, the call per iteration, and what it found."""
    out = {}
    for metric in ("point", "plane"):
        dc.align_reference(ref, max_distance=reach, max_iterations=2, metric=metric)  # warm-up
        runs = [timed(lambda: dc.align_reference(ref, max_distance=reach, max_iterations=iterations, metric=metric)) for _ in range(repeats)]
        got = runs[0][1]
        assert all(r[1]["transform"].tobytes() == got["transform"].tobytes() and r[1]["history"] == got["history"] for r in runs)  # the same bytes every run
        h = got["history"]
        out[metric] = {"align_reference": spread([r[0] for r in runs]), "align_reference_per_iteration": spread([r[0] / got["iterations"] for r in runs]),
                       "iterations": got["iterations"], "stop": got["stop"], "pairs_first_iteration": h[0]["matched"], "rms_first_m": h[0]["rms_m"], "rms_last_m": h[-1]["rms_m"],
                       "shift_last_m": h[-1]["shift_m"], "rotation_last_rad": h[-1]["rotation_rad"],
                       "largest_entry_error_against_the_applied_motion": float(np.abs(got["transform"] - motion).max())}
        if metric == "plane":
            out[metric].update({"used_first_iteration": h[0]["used"], "no_normal_first_iteration": h[0]["no_normal"], "plane_rms_first_m": h[0]["plane_rms_m"],
                                "plane_rms_last_m": h[-1]["plane_rms_m"], "smallest_min_pivot": min(x["min_pivot"] for x in h)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--min-range", type=float, default=0.5)
    ap.add_argument("--degrees", type=float, default=0.5)
    ap.add_argument("--metres", type=float, default=0.05)
    ap.add_argument("--normals-radius", type=float, default=0.3)
    ap.add_argument("--kernels-only", action="store_true", help="the stage calls alone, for a profiler run")
    ap.add_argument("--trace", help="the output directory of a rocprofv3 --kernel-trace run of --kernels-only: its per-kernel figures are merged into --out")
    ap.add_argument("--out", help="JSON file the figures are written to (merged into what it already holds)")
    a = ap.parse_args()
    result = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    if a.trace:
        result["kernels_from_one_kernel_trace_run"] = trace_figures(a.trace)
    else:
        from dmsa_lidar_slam_amd import raw_sequence as rs
        from dmsa_lidar_slam_amd import _capi as capi
        from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator, align_plane_solve, align_solve

        scale_c = float(capi.load_library().dmsa_dense_align_scale(a.voxel))
        with tempfile.TemporaryDirectory() as tmp:
            dump, poses, _ = dct.make_sequence(tmp, a.messages, a.points)
            dc = DenseCloudCreator.from_tum_file(poses, DenseCloudConfig(minRange=a.min_range, voxelSize=a.voxel), retain=True)
            for kind, msg in rs.RawReader(dump):
                if kind == "pointcloud2":
                    dc.add_pointcloud2(msg, "ouster", download=False)
            g, _ = dc.retained()
            n = g.shape[0]
            centre = g[:, :3].mean(axis=0).astype(np.float64)
            motion = rigid(a.degrees, (0.2, -0.3, 1.0), (0.6 * a.metres, -0.48 * a.metres, 0.64 * a.metres))
            motion[:, 3] += centre - motion[:, :3] @ centre  # the rotation is about the cloud's centre
            inv = np.concatenate([motion[:, :3].T, -(motion[:, :3].T @ motion[:, 3:])], axis=1)
            jittered = g[:, :3].astype(np.float64) + np.random.default_rng(21).uniform(-0.5, 0.5, (n, 3)) * a.voxel
            ref = (jittered @ inv[:, :3].T + inv[:, 3]).astype(np.float32)
            dc.compute_normals(radius=a.normals_radius, download=False)  # warm-up
            normals = [timed(lambda: dc.compute_normals(radius=a.normals_radius, download=False)) for _ in range(a.repeats)]
            figures = {"compute_normals": spread([t for t, _ in normals]), "rows_without_a_normal": normals[0][1][1]}
            for reach in REACHES:
                dc.set_reference(ref, np.eye(3, 4))
                dc.align_sums(reach), dc.align_plane_sums(reach)  # warm-up: both grids at this edge
                point, plane = [], []
                for _ in range(a.repeats):
                    t, sums = timed(lambda: dc.align_sums(reach))
                    point.append(t)
                    t, psums = timed(lambda: dc.align_plane_sums(reach))
                    plane.append(t)
                entry = {"align_sums_grids_kept": spread(point), "align_plane_sums_grids_kept": spread(plane),
                         "plane_minus_point_stage_call_s": round(statistics.median(plane) - statistics.median(point), 5)}
                if not a.kernels_only:
                    entry.update({"align_solve_host": spread([timed(lambda: align_solve(sums, scale_c))[0] for _ in range(a.repeats)]),
                                  "align_plane_solve_host": spread([timed(lambda: align_plane_solve(psums, scale_c))[0] for _ in range(a.repeats)])})
                    entry.update(both_metrics(dc, ref, reach, a.repeats, motion))
                figures[f"max_distance_{reach:g}"] = entry
            dc.close()
        result.update({"workload": {"messages": a.messages, "points_per_message": a.points, "voxel_size": a.voxel, "min_range": a.min_range, "retained_rows": n,
                                    "reference_rows": n, "degrees": a.degrees, "metres": a.metres, "normals_radius": a.normals_radius,
                                    "reference": "the store, every row displaced by a fixed pseudo-random offset below half a voxel per axis, then moved by the inverse of the motion",
                                    "note": "a jittered copy of a voxel-thinned cloud fills a volume: its normals mean little, nothing is claimed of the plane call's convergence here"},
                       "device": figures})
        if not a.kernels_only:
            import dense_align_model as am
            from test_gpu_dense_normals import _still_cloud

            from dmsa_lidar_slam_amd.api import DmsaOptimizer

            opt = DmsaOptimizer(device=0)
            rng = np.random.default_rng(5)
            dc, _ = _still_cloud(opt, am.room(rng), 0.1)
            g, _ = dc.retained()
            _, without = dc.compute_normals(radius=a.normals_radius, download=False)
            room = {"store_rows": int(g.shape[0]), "reference_rows": 2000, "noise_m": 0.01, "rows_without_a_normal": without}
            for deg, shift in ((2.0, (0.1, -0.08, 0.07)), (5.0, (0.25, -0.2, 0.18))):
                m = am.rigid(deg, (0.2, -0.3, 1.0), shift)
                room[f"{deg:g}_degrees"] = both_metrics(dc, am.sample_reference(rng, g, 2000, 0.01, m), 1.0, a.repeats, m)
            result["room"] = room
            dc.close()
            opt.close()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
