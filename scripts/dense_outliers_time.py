"""Time of the dense cloud's statistical outlier removal (include/dmsa_dense_outliers.h) on the workload of profiles/r09_dense_cloud.json: 200
Ouster messages of 131 072 points, voxel 0.1 m; k = 8, radius 0.3 m, stddev_mul 1.

    python scripts/dense_outliers_time.py --out profiles/r12_dense_outliers.json

End to end is the time from "the retained store is complete" to "the x y z file of the cleaned store is written":
dmsa_dense_cloud_classify_outliers (cell keys, sort, cell table, k_knn_mean_distance, the sums, the flags and their scan),
dmsa_dense_cloud_remove_outliers and dmsa_dense_cloud_save_pcd_retained to /dev/null, each ending in a host wait; median of 5 after a warm-up.
remove_outliers changes the store, so every run fills a fresh object from the same dump (not timed), and its first classification builds its
own grid.  Filling the store is the dense cloud itself (profiles/r09_dense_cloud.json) and is reported beside the figures, not inside them.
The host figure is ONE thread doing O2-O5 over a hash grid (std::unordered_map of cell -> rows, 27 cells per query, the same float test, a
sorted list of the k smallest d2 per query, the same integer sums and the same O5) on the same retained points -- a small C++ helper this
script builds -- over the first --baseline-rows rows, scaled per row; its mean distances are compared with the device's bit for bit.  No
threshold is fixed in advance."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_cloud_time as dct  # noqa: E402  (the sequence generator)
from dense_normals_time import spread, timed  # noqa: E402

BASELINE_SRC = r"""
#include <chrono>
#include <cmath>
#include <cstdint>
#include <limits>
#include <unordered_map>
#include <vector>
// O2-O4 of dmsa_dense_outliers.h on one thread: g as float4 rows; m_i of rows [0, rows) against all n points, and their three sums
extern "C" void baseline_outliers(const float* g, long long n, long long rows, float radius, int k, float* mean, long long* sums /* n_s, S1, S2, isolated */,
                                  double* seconds /* grid, rows */) {
    const auto t0 = std::chrono::steady_clock::now();
    const double cell = 1.001 * (double)radius;
    auto key_of = [&](long long x, long long y, long long z) { return (uint64_t)(x + 1048576) << 42 | (uint64_t)(y + 1048576) << 21 | (uint64_t)(z + 1048576); };
    std::unordered_map<uint64_t, std::vector<uint32_t>> grid;
    grid.reserve((size_t)n / 4);
    for (long long i = 0; i < n; ++i)
        grid[key_of((long long)std::floor(g[4 * i] / cell), (long long)std::floor(g[4 * i + 1] / cell), (long long)std::floor(g[4 * i + 2] / cell))].push_back((uint32_t)i);
    const auto t1 = std::chrono::steady_clock::now();
    int e = 0;
    (void)std::frexp(radius, &e);
    const float scale = std::ldexp(1.0f, 18 - e), r2 = radius * radius;
    sums[0] = sums[1] = sums[2] = sums[3] = 0;
    for (long long i = 0; i < rows; ++i) {
        const float qx = g[4 * i], qy = g[4 * i + 1], qz = g[4 * i + 2];
        const long long cx = (long long)std::floor(qx / cell), cy = (long long)std::floor(qy / cell), cz = (long long)std::floor(qz / cell);
        float best[16];
        for (int s = 0; s < k; ++s) best[s] = std::numeric_limits<float>::infinity();
        for (long long x = cx - 1; x <= cx + 1; ++x)
            for (long long y = cy - 1; y <= cy + 1; ++y)
                for (long long z = cz - 1; z <= cz + 1; ++z) {
                    const auto it = grid.find(key_of(x, y, z));
                    if (it == grid.end()) continue;
                    for (const uint32_t j : it->second) {
                        const float dx = g[4 * j] - qx, dy = g[4 * j + 1] - qy, dz = g[4 * j + 2] - qz;
                        float d2 = dx * dx;
                        d2 += dy * dy;
                        d2 += dz * dz;
                        if (!(d2 <= r2) || (long long)j == i || !(d2 < best[k - 1])) continue;
                        int s = k - 1;
                        for (; s > 0 && d2 < best[s - 1]; --s) best[s] = best[s - 1];
                        best[s] = d2;
                    }
                }
        if (!(best[k - 1] <= r2)) {
            mean[i] = std::numeric_limits<float>::quiet_NaN();
            ++sums[3];
            continue;
        }
        float sum = std::sqrt(best[0]);
        for (int s = 1; s < k; ++s) sum += std::sqrt(best[s]);
        mean[i] = sum / (float)k;
        const long long q = (long long)std::rint(mean[i] * scale);
        sums[0] += 1, sums[1] += q, sums[2] += q * q;
    }
    seconds[0] = std::chrono::duration<double>(t1 - t0).count(), seconds[1] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
}
"""


def build_baseline(tmp):
    src, lib = os.path.join(tmp, "outliers_baseline.cpp"), os.path.join(tmp, "liboutliers_baseline.so")
    with open(src, "w") as f:
        f.write(BASELINE_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    L.baseline_outliers.restype = None
    L.baseline_outliers.argtypes = [C.POINTER(C.c_float), C.c_longlong, C.c_longlong, C.c_float, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    return L


def run_baseline(L, g, rows, radius, k):
    """(m of the first `rows` rows, (n_s, S1, S2, isolated) over them, seconds for the grid, seconds for the rows)."""
    g = np.ascontiguousarray(g, np.float32)
    mean, sums, sec = np.zeros(rows, np.float32), (C.c_longlong * 4)(), (C.c_double * 2)()
    L.baseline_outliers(g.ctypes.data_as(C.POINTER(C.c_float)), g.shape[0], rows, float(np.float32(radius)), k, mean.ctypes.data_as(C.POINTER(C.c_float)), sums, sec)
    return mean, tuple(int(v) for v in sums), float(sec[0]), float(sec[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--min-range", type=float, default=0.5)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--mul", type=float, default=1.0)
    ap.add_argument("--baseline-rows", type=int, default=300000, help="rows the one-thread host figure computes (against all retained points)")
    ap.add_argument("--out", help="JSON file the figures are written to (merged into what it already holds)")
    a = ap.parse_args()
    result = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    from dmsa_lidar_slam_amd import raw_sequence as rs
    from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator, outlier_threshold

    with tempfile.TemporaryDirectory() as tmp:
        dump, poses, _ = dct.make_sequence(tmp, a.messages, a.points)

        def filled():
            dc = DenseCloudCreator.from_tum_file(poses, DenseCloudConfig(minRange=a.min_range, voxelSize=a.voxel), retain=True)
            sec, _ = timed(lambda: [dc.add_pointcloud2(msg, "ouster", download=False) for kind, msg in rs.RawReader(dump) if kind == "pointcloud2"])
            return dc, sec

        def one_run(path):
            dc, fill_s = filled()
            n = dc.retained_count()
            t_classify, stats = timed(lambda: dc.classify_outliers(a.radius, a.k, a.mul))
            t_remove, left = timed(dc.remove_outliers)
            t_save, (points, size) = timed(lambda: dc.save_pcd_retained(path))
            dc.close()
            assert points == left == stats["inliers"] and stats["rows"] == n
            return t_classify, t_remove, t_save, stats, size, fill_s

        figures = {}
        for tag, path in (("dev_null", "/dev/null"), ("local_file", os.path.join(tmp, "clean.pcd"))):
            one_run(path)  # warm-up: code objects, page cache
            runs = [one_run(path) for _ in range(a.repeats)]
            figures[tag] = {"classify_outliers": spread([r[0] for r in runs]), "remove_outliers": spread([r[1] for r in runs]), "save_pcd_retained": spread([r[2] for r in runs]),
                            "end_to_end": spread([r[0] + r[1] + r[2] for r in runs]), "file_bytes": runs[0][4]}
            figures[tag]["rows_per_s"] = round(runs[0][3]["rows"] / figures[tag]["end_to_end"]["median_s"])
            assert all(r[3] == runs[0][3] for r in runs)  # the same integers and the same doubles every run
        stats, fill_s = runs[0][3], runs[0][5]
        # the one-thread host figure on the same retained points
        dc, _ = filled()
        g, _ = dc.retained()
        n = g.shape[0]
        rows = min(a.baseline_rows, n)
        device_mean = dc.knn_mean_distance(a.radius, a.k, 0, rows)
        dc.close()
        mean, sums, grid_s, rows_s = run_baseline(build_baseline(tmp), g, rows, a.radius, a.k)
        t_threshold, _ = timed(lambda: outlier_threshold(sums[0], sums[1], sums[2], a.mul))
        result.update({
            "workload": {"messages": a.messages, "points_per_message": a.points, "voxel_size": a.voxel, "min_range": a.min_range, "radius": a.radius, "k": a.k,
                         "stddev_mul": a.mul, "retained_rows": n, "fill_store_s": round(fill_s, 3)},
            "classification": stats,
            "device": figures,
            "host_one_thread": {"rows": rows, "grid_s": round(grid_s, 3), "rows_s": round(rows_s + t_threshold, 3), "rows_per_s": round(rows / rows_s),
                                "scaled_to_all_rows_s": round(grid_s + rows_s * n / rows, 1), "isolated_in_rows": sums[3],
                                "mean_distances_equal_device_bits": bool(np.array_equal(mean.view(np.uint32), device_mean.view(np.uint32)))},
        })
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
