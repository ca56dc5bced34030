"""Time of the dense cloud's Euclidean clustering (include/dmsa_dense_clusters.h) on the workload of profiles/r09_dense_cloud.json: 200 Ouster
messages of 131 072 points, voxel 0.1 m; radius 0.3 m, min_size 50.

    python scripts/dense_clusters_time.py --out profiles/r20_dense_clusters.json

End to end is the time from "the retained store is complete" to "the x y z file of the cleaned store is written":
dmsa_dense_cloud_classify_clusters (cell keys, sort, cell table, k_cluster_link, the flattening, sizes, labels, the flags and their scan),
dmsa_dense_cloud_remove_clusters and dmsa_dense_cloud_save_pcd_retained, each ending in a host wait; median of 5 after a warm-up.  The
x y z label file of the whole store (dmsa_dense_cloud_save_pcd_labels, before the removal) is timed beside them.  remove_clusters changes the
store, so every run fills a fresh object from the same dump (not timed), and its classification builds its own grid.
dmsa_dense_cloud_classify_outliers at k = 8 is timed in the same process on fresh objects of the same store: the same traversal of the same
grid with a list of distances where this stage has a union-find.
The host figure is ONE thread doing C2-C5 over a hash grid (std::unordered_map of cell -> rows, 27 cells per row, the same float test, a
union-find with path halving in which the larger root hooks under the smaller) on the same retained points -- a small C++ helper this script
builds -- over ALL rows; its labels and sizes are compared with the device's.  No threshold is fixed in advance."""
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
#include <unordered_map>
#include <vector>
// C2-C4 of dmsa_dense_clusters.h on one thread: g as float4 rows; label, size and keep of all n rows
extern "C" void baseline_clusters(const float* g, long long n, float radius, int min_size, int max_size, int* label, int* size, unsigned char* keep,
                                  double* seconds /* grid, union-find, labels and flags */) {
    const auto t0 = std::chrono::steady_clock::now();
    const double cell = 1.001 * (double)radius;
    auto key_of = [&](long long x, long long y, long long z) { return (uint64_t)(x + 1048576) << 42 | (uint64_t)(y + 1048576) << 21 | (uint64_t)(z + 1048576); };
    std::unordered_map<uint64_t, std::vector<uint32_t>> grid;
    grid.reserve((size_t)n / 4);
    for (long long i = 0; i < n; ++i)
        grid[key_of((long long)std::floor(g[4 * i] / cell), (long long)std::floor(g[4 * i + 1] / cell), (long long)std::floor(g[4 * i + 2] / cell))].push_back((uint32_t)i);
    const auto t1 = std::chrono::steady_clock::now();
    const float r2 = radius * radius;
    std::vector<uint32_t> parent((size_t)n);
    for (long long i = 0; i < n; ++i) parent[i] = (uint32_t)i;
    auto find = [&](uint32_t x) {
        while (parent[x] != x) {
            parent[x] = parent[parent[x]];
            x = parent[x];
        }
        return x;
    };
    for (long long i = 0; i < n; ++i) {
        const float qx = g[4 * i], qy = g[4 * i + 1], qz = g[4 * i + 2];
        const long long cx = (long long)std::floor(qx / cell), cy = (long long)std::floor(qy / cell), cz = (long long)std::floor(qz / cell);
        for (long long x = cx - 1; x <= cx + 1; ++x)
            for (long long y = cy - 1; y <= cy + 1; ++y)
                for (long long z = cz - 1; z <= cz + 1; ++z) {
                    const auto it = grid.find(key_of(x, y, z));
                    if (it == grid.end()) continue;
                    for (const uint32_t j : it->second) {
                        if ((long long)j >= i) continue;  // every pair once
                        const float dx = g[4 * j] - qx, dy = g[4 * j + 1] - qy, dz = g[4 * j + 2] - qz;
                        float d2 = dx * dx;
                        d2 += dy * dy;
                        d2 += dz * dz;
                        if (!(d2 <= r2)) continue;
                        const uint32_t a = find((uint32_t)i), b = find(j);
                        if (a < b) parent[b] = a;
                        else if (b < a) parent[a] = b;
                    }
                }
    }
    const auto t2 = std::chrono::steady_clock::now();
    for (long long i = 0; i < n; ++i) size[i] = 0;
    for (long long i = 0; i < n; ++i) label[i] = (int)find((uint32_t)i), ++size[label[i]];
    for (long long i = 0; i < n; ++i) size[i] = size[label[i]];  // (only roots were counted into, and a root reads itself)
    for (long long i = 0; i < n; ++i) keep[i] = size[i] >= min_size && (max_size == 0 || size[i] <= max_size);
    const auto t3 = std::chrono::steady_clock::now();
    seconds[0] = std::chrono::duration<double>(t1 - t0).count(), seconds[1] = std::chrono::duration<double>(t2 - t1).count();
    seconds[2] = std::chrono::duration<double>(t3 - t2).count();
}
"""


def build_baseline(tmp):
    src, lib = os.path.join(tmp, "clusters_baseline.cpp"), os.path.join(tmp, "libclusters_baseline.so")
    with open(src, "w") as f:
        f.write(BASELINE_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    L.baseline_clusters.restype = None
    L.baseline_clusters.argtypes = [C.POINTER(C.c_float), C.c_longlong, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ubyte),
                                    C.POINTER(C.c_double)]
    return L


def run_baseline(L, g, radius, min_size, max_size):
    """(label, size, keep of all rows, seconds for the grid, for the union-find, for labels and flags)."""
    g = np.ascontiguousarray(g, np.float32)
    n = g.shape[0]
    label, size, keep, sec = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8), (C.c_double * 3)()
    L.baseline_clusters(g.ctypes.data_as(C.POINTER(C.c_float)), n, float(np.float32(radius)), min_size, max_size, label.ctypes.data_as(C.POINTER(C.c_int)),
                        size.ctypes.data_as(C.POINTER(C.c_int)), keep.ctypes.data_as(C.POINTER(C.c_ubyte)), sec)
    return label, size, keep, float(sec[0]), float(sec[1]), float(sec[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--min-range", type=float, default=0.5)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--min-size", type=int, default=50)
    ap.add_argument("--max-size", type=int, default=0)
    ap.add_argument("--outlier-k", type=int, default=8)
    ap.add_argument("--out", help="JSON file the figures are written to (merged into what it already holds)")
    a = ap.parse_args()
    result = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    from dmsa_lidar_slam_amd import raw_sequence as rs
    from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator

    with tempfile.TemporaryDirectory() as tmp:
        dump, poses, _ = dct.make_sequence(tmp, a.messages, a.points)

        def filled():
            dc = DenseCloudCreator.from_tum_file(poses, DenseCloudConfig(minRange=a.min_range, voxelSize=a.voxel), retain=True)
            sec, _ = timed(lambda: [dc.add_pointcloud2(msg, "ouster", download=False) for kind, msg in rs.RawReader(dump) if kind == "pointcloud2"])
            return dc, sec

        def one_run(path, labels_path):
            dc, fill_s = filled()
            n = dc.retained_count()
            t_classify, stats = timed(lambda: dc.classify_clusters(a.radius, a.min_size, a.max_size))
            t_labels, (l_points, l_size) = timed(lambda: dc.save_pcd_labels(labels_path))
            t_remove, left = timed(dc.remove_clusters)
            t_save, (points, size) = timed(lambda: dc.save_pcd_retained(path))
            dc.close()
            assert points == left == stats["kept_rows"] and stats["rows"] == n == l_points
            return t_classify, t_remove, t_save, stats, size, fill_s, t_labels, l_size

        def outliers_run():
            dc, _ = filled()
            t, stats = timed(lambda: dc.classify_outliers(a.radius, a.outlier_k, 1.0))
            dc.close()
            return t, stats["rows"]

        figures = {}
        for tag, path, labels_path in (("dev_null", "/dev/null", "/dev/null"), ("local_file", os.path.join(tmp, "clean.pcd"), os.path.join(tmp, "labels.pcd"))):
            one_run(path, labels_path)  # warm-up: code objects, page cache
            runs = [one_run(path, labels_path) for _ in range(a.repeats)]
            figures[tag] = {"classify_clusters": spread([r[0] for r in runs]), "remove_clusters": spread([r[1] for r in runs]), "save_pcd_retained": spread([r[2] for r in runs]),
                            "end_to_end": spread([r[0] + r[1] + r[2] for r in runs]), "file_bytes": runs[0][4], "save_pcd_labels": spread([r[6] for r in runs]),
                            "labels_file_bytes": runs[0][7]}
            figures[tag]["rows_per_s"] = round(runs[0][3]["rows"] / figures[tag]["end_to_end"]["median_s"])
            assert all(r[3] == runs[0][3] for r in runs)  # the same integers every run
        stats, fill_s = runs[0][3], runs[0][5]
        outliers_run()
        o_runs = [outliers_run() for _ in range(a.repeats)]
        knn = spread([r[0] for r in o_runs])
        # the one-thread host figure on the same retained points
        dc, _ = filled()
        g, _ = dc.retained()
        n = g.shape[0]
        t_label_call, (device_label, device_size) = timed(lambda: dc.cluster_labels(a.radius))
        dc.close()
        label, size, keep, grid_s, unite_s, rest_s = run_baseline(build_baseline(tmp), g, a.radius, a.min_size, a.max_size)
        host_s = grid_s + unite_s + rest_s
        classify_s = figures["dev_null"]["classify_clusters"]["median_s"]
        result.update({
            "workload": {"messages": a.messages, "points_per_message": a.points, "voxel_size": a.voxel, "min_range": a.min_range, "radius": a.radius,
                         "min_size": a.min_size, "max_size": a.max_size, "retained_rows": n, "fill_store_s": round(fill_s, 3)},
            "classification": stats,
            "device": figures,
            "cluster_labels_with_download_s": round(t_label_call, 4),
            "classify_outliers_same_store": {"k": a.outlier_k, **knn},
            "classify_clusters_over_classify_outliers": round(classify_s / knn["median_s"], 2),
            "host_one_thread": {"rows": n, "grid_s": round(grid_s, 3), "union_find_s": round(unite_s, 3), "labels_and_flags_s": round(rest_s, 3), "total_s": round(host_s, 3),
                                "over_device_classify": round(host_s / classify_s, 1), "kept_rows": int(keep.sum()),
                                "labels_equal_device": bool(np.array_equal(label, device_label)), "sizes_equal_device": bool(np.array_equal(size, device_size))},
        })
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
