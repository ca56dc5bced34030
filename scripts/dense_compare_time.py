"""Time of the dense cloud's comparison with a reference cloud (include/dmsa_dense_compare.h) on the workload of profiles/r09_dense_cloud.json:
200 Ouster messages of 131 072 points, voxel 0.1 m.  The reference is the retained store itself with every row displaced by a fixed
pseudo-random offset below one voxel per axis, so every query has work to do.  max_distance 0.3 m and again 1.0 m, tolerance 0.1 m.

    python scripts/dense_compare_time.py --out profiles/r21_dense_compare.json
    rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- python scripts/dense_compare_time.py --kernels-only
    python scripts/dense_compare_time.py --trace DIR --out profiles/r21_dense_compare.json

The first form times, each as a median of 5 after a warm-up and each ending in a host wait: dmsa_dense_cloud_set_reference (the upload, the
validity kernel), dmsa_dense_cloud_compare end to end (both search grids on its first call at an edge, both directions, the sums, one host
read), and in the same process dmsa_dense_cloud_classify_outliers at k = 8 and radius 0.3 on a fresh object of the same store: the comparable
walker.  It also times ONE host thread doing D2 of the accuracy direction over a hash grid (std::unordered_map of cell -> rows, 27 cells per
query, the same float arithmetic; a small C++ helper this script builds) on a 2 % SAMPLE of the store's rows, SCALED by 50 and labelled as
such, and requires its indices and q to equal the device's on the sample.
The second form is the work of the first without the host figure, for a profiler run of its own; the third reads that run's kernel trace:
per dispatch of k_nearest_across in launch order (accuracy, completeness; the warm-up left out) and of k_knn_mean_distance, medians.
No threshold is fixed in advance."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_cloud_time as dct  # noqa: E402  (the sequence generator)
from dense_normals_time import spread, timed  # noqa: E402

REACHES = (0.3, 1.0)

BASELINE_SRC = r"""
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>
// D2 and q of dmsa_dense_compare.h on one thread: the queries q (3 floats each) against the rows s (3 floats each)
extern "C" void baseline_nearest(const float* q, long long nq, const float* s, long long ns, float reach, float scale, int* index, int* quant,
                                 double* seconds /* grid, search */) {
    const auto t0 = std::chrono::steady_clock::now();
    const double cell = 1.001 * (double)reach;
    auto key_of = [&](long long x, long long y, long long z) { return (uint64_t)(x + 1048576) << 42 | (uint64_t)(y + 1048576) << 21 | (uint64_t)(z + 1048576); };
    std::unordered_map<uint64_t, std::vector<uint32_t>> grid;
    grid.reserve((size_t)ns / 4);
    for (long long i = 0; i < ns; ++i)
        grid[key_of((long long)std::floor(s[3 * i] / cell), (long long)std::floor(s[3 * i + 1] / cell), (long long)std::floor(s[3 * i + 2] / cell))].push_back((uint32_t)i);
    const auto t1 = std::chrono::steady_clock::now();
    const float r2 = reach * reach;
    for (long long i = 0; i < nq; ++i) {
        const float qx = q[3 * i], qy = q[3 * i + 1], qz = q[3 * i + 2];
        const long long cx = (long long)std::floor(qx / cell), cy = (long long)std::floor(qy / cell), cz = (long long)std::floor(qz / cell);
        uint64_t best = ~0ull;
        for (long long x = cx - 1; x <= cx + 1; ++x)
            for (long long y = cy - 1; y <= cy + 1; ++y)
                for (long long z = cz - 1; z <= cz + 1; ++z) {
                    const auto it = grid.find(key_of(x, y, z));
                    if (it == grid.end()) continue;
                    for (const uint32_t j : it->second) {
                        const float dx = s[3 * j] - qx, dy = s[3 * j + 1] - qy, dz = s[3 * j + 2] - qz;
                        float d2 = dx * dx;
                        d2 += dy * dy;
                        d2 += dz * dz;
                        if (!(d2 <= r2)) continue;
                        uint32_t bits;
                        std::memcpy(&bits, &d2, 4);
                        const uint64_t k = (uint64_t)bits << 32 | j;
                        if (k < best) best = k;
                    }
                }
        index[i] = -1, quant[i] = -1;
        if (best != ~0ull) {
            const uint32_t bits = (uint32_t)(best >> 32);
            float d2;
            std::memcpy(&d2, &bits, 4);
            index[i] = (int)(uint32_t)best, quant[i] = (int)std::rint(std::sqrt(d2) * scale);
        }
    }
    const auto t2 = std::chrono::steady_clock::now();
    seconds[0] = std::chrono::duration<double>(t1 - t0).count(), seconds[1] = std::chrono::duration<double>(t2 - t1).count();
}
"""


def build_baseline(tmp):
    src, lib = os.path.join(tmp, "compare_baseline.cpp"), os.path.join(tmp, "libcompare_baseline.so")
    with open(src, "w") as f:
        f.write(BASELINE_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    L.baseline_nearest.restype = None
    L.baseline_nearest.argtypes = [C.POINTER(C.c_float), C.c_longlong, C.POINTER(C.c_float), C.c_longlong, C.c_float, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_double)]
    return L


def run_baseline(L, q, s, reach, scale):
    q, s = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(s, np.float32)
    index, quant, sec = np.zeros(q.shape[0], np.int32), np.zeros(q.shape[0], np.int32), (C.c_double * 2)()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    L.baseline_nearest(fp(q), q.shape[0], fp(s), s.shape[0], float(np.float32(reach)), float(scale), index.ctypes.data_as(C.POINTER(C.c_int)),
                       quant.ctypes.data_as(C.POINTER(C.c_int)), sec)
    return index, quant, float(sec[0]), float(sec[1])


def trace_figures(directory):
    """Durations [ms] per dispatch from the *kernel_trace.csv of a rocprofv3 --kernel-trace run, in launch order."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6) for r in csv.DictReader(open(path))]
    rows.sort()
    of = lambda name: [ms for _, kernel, ms in rows if name in kernel]
    near, out = of("k_nearest_across"), {}
    per_reach = len(near) // len(REACHES)  # (warm-up + repeats) x two directions
    for k, reach in enumerate(REACHES):
        mine = near[k * per_reach + 2 : (k + 1) * per_reach]  # (the warm-up's two dispatches left out)
        out[f"max_distance_{reach:g}"] = {"k_nearest_across_accuracy_ms": round(statistics.median(mine[0::2]), 3), "k_nearest_across_completeness_ms": round(statistics.median(mine[1::2]), 3),
                                          "dispatches": len(mine)}
    for name in ("k_compare_quantise_sum", "k_reference_transform", "k_reference_cell_keys", "k_knn_mean_distance", "k_outlier_quantise_sum"):
        if of(name):
            out[name + "_ms"] = {"median": round(statistics.median(of(name)), 3), "min": round(min(of(name)), 3), "max": round(max(of(name)), 3), "dispatches": len(of(name))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--min-range", type=float, default=0.5)
    ap.add_argument("--tolerance", type=float, default=0.1)
    ap.add_argument("--outlier-k", type=int, default=8)
    ap.add_argument("--sample", type=float, default=0.02, help="share of the store's rows the one-thread host figure is measured on")
    ap.add_argument("--kernels-only", action="store_true", help="the device work alone, for a profiler run")
    ap.add_argument("--trace", help="the output directory of a rocprofv3 --kernel-trace run of --kernels-only: its per-kernel figures are merged into --out")
    ap.add_argument("--out", help="JSON file the figures are written to (merged into what it already holds)")
    a = ap.parse_args()
    result = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    if a.trace:
        result["kernels_from_one_kernel_trace_run"] = trace_figures(a.trace)
    else:
        from dmsa_lidar_slam_amd import raw_sequence as rs
        from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator

        with tempfile.TemporaryDirectory() as tmp:
            dump, poses, _ = dct.make_sequence(tmp, a.messages, a.points)

            def filled():
                dc = DenseCloudCreator.from_tum_file(poses, DenseCloudConfig(minRange=a.min_range, voxelSize=a.voxel), retain=True)
                for kind, msg in rs.RawReader(dump):
                    if kind == "pointcloud2":
                        dc.add_pointcloud2(msg, "ouster", download=False)
                return dc

            dc = filled()
            g, _ = dc.retained()
            n = g.shape[0]
            ref = (g[:, :3] + np.random.default_rng(21).uniform(-0.5, 0.5, (n, 3)) * a.voxel).astype(np.float32)
            dc.set_reference(ref)  # warm-up
            upload = spread([timed(lambda: dc.set_reference(ref))[0] for _ in range(a.repeats)])
            figures = {}
            for reach in REACHES:
                first_s, stats = timed(lambda: dc.compare(reach, a.tolerance))  # builds both grids at this edge
                runs = [timed(lambda: dc.compare(reach, a.tolerance)) for _ in range(a.repeats)]
                assert all(r[1] == stats for r in runs)  # the same integers and doubles every run
                acc, com = stats["accuracy"], stats["completeness"]
                figures[f"max_distance_{reach:g}"] = {
                    "compare_first_call_with_both_grids_s": round(first_s, 4), "compare": spread([r[0] for r in runs]),
                    "accuracy": {k: acc[k] for k in ("matched", "unmatched", "within", "mean_m", "rms_m")},
                    "completeness": {k: com[k] for k in ("matched", "unmatched", "within", "mean_m", "rms_m")},
                    "precision": stats["precision"], "recall": stats["recall"], "f_score": stats["f_score"]}
            other = filled()
            other.classify_outliers(0.3, a.outlier_k, 1.0)  # warm-up, and the grid
            knn = spread([timed(lambda: other.classify_outliers(0.3, a.outlier_k, 1.0))[0] for _ in range(a.repeats)])
            other.close()
            result.update({"workload": {"messages": a.messages, "points_per_message": a.points, "voxel_size": a.voxel, "min_range": a.min_range, "tolerance": a.tolerance,
                                        "retained_rows": n, "reference_rows": n, "reference": "the store, every row displaced by a fixed pseudo-random offset below half a voxel per axis"},
                           "set_reference": upload, "device": figures, "classify_outliers_same_store_grid_kept": {"k": a.outlier_k, "radius": 0.3, **knn}})
            if not a.kernels_only:
                L = build_baseline(tmp)
                pick = np.sort(np.random.default_rng(5).choice(n, max(1, int(n * a.sample)), replace=False))
                host = {}
                for reach in REACHES:
                    scale = dc.compare(reach, a.tolerance)["scale"]
                    dist, index = dc.nearest_in_reference(reach)
                    index_h, quant_h, grid_s, search_s = run_baseline(L, g[pick, :3], ref, reach, scale)
                    with np.errstate(invalid="ignore"):
                        quant_d = np.where(index[pick] >= 0, np.rint(dist[pick] * np.float32(scale)), -1).astype(np.int32)
                    device_s = figures[f"max_distance_{reach:g}"]["compare"]["median_s"]
                    host[f"max_distance_{reach:g}"] = {
                        "sample_rows": int(pick.shape[0]), "grid_of_all_reference_rows_s": round(grid_s, 3), "search_of_the_sample_s": round(search_s, 3),
                        "one_direction_scaled_to_all_rows_s": round(grid_s + search_s / a.sample, 1), "scaled": f"the search time of a {a.sample:g} sample divided by {a.sample:g}",
                        "both_directions_scaled_over_device_compare": round(2 * (grid_s + search_s / a.sample) / device_s, 1),
                        "indices_equal_device_on_sample": bool(np.array_equal(index_h, index[pick])), "q_equal_device_on_sample": bool(np.array_equal(quant_h, quant_d))}
                    assert host[f"max_distance_{reach:g}"]["indices_equal_device_on_sample"] and host[f"max_distance_{reach:g}"]["q_equal_device_on_sample"]
                result["host_one_thread_accuracy_direction"] = host
            dc.close()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
