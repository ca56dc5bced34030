"""Time of the dense cloud's normals (include/dmsa_dense_normals.h) on the workload of profiles/r09_dense_cloud.json: 200 Ouster messages of
131 072 points, voxel 0.1 m, radius 0.3 m.

    python scripts/dense_normals_time.py --out profiles/r10_dense_normals.json --keep DIR       end to end + the one-thread host figure
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR2 -o normals -- examples/dense_cloud_from_raw DIR/sequence.raw DIR/Poses.txt ouster /dev/null 0.3 --voxel 0.1 --min-range 0.5
    python scripts/dense_normals_time.py --kernel-stats DIR2 --out profiles/r10_dense_normals.json    adds the kernel split of that run
    rocprofv3 --pmc <counters> --output-format csv -d DIR3 -o pmc -- examples/dense_cloud_from_raw ... (a run of its own, no tracing)
    python scripts/dense_normals_time.py --pmc DIR3 --out profiles/r10_dense_normals.json             adds the counters of k_neighbour_moments

End to end is the time from "the retained store is complete" to "the seven-field file is written": dmsa_dense_cloud_compute_normals (cell
keys, sort, cell table, moments, normals) followed by dmsa_dense_cloud_save_pcd_normals to /dev/null, each ending in a host wait; median
of 5 after a warm-up.  Before every timed run the grid is rebuilt for another radius, so that the timed call builds its own.  Filling the
store is the dense cloud itself (profiles/r09_dense_cloud.json) and is reported beside it, not inside it.
The host figure is ONE thread doing N2-N4 over a hash grid (std::unordered_map of cell -> rows, 27 cells per query, the same float test, the
same integer sums, N4 through the same csrc/pcl_eigen33.h) on the same retained points -- a small C++ helper this script builds -- over the
first --baseline-rows rows, scaled per row; its normals are compared with the device's bit for bit.  No threshold is fixed in advance."""
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
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_cloud_time as dct  # noqa: E402  (the sequence generator and the reader of a profiler run)

BASELINE_SRC = r"""
#include <chrono>
#include <cmath>
#include <cstdint>
#include <unordered_map>
#include <vector>
#include "pcl_eigen33.h"
// N2-N4 of dmsa_dense_normals.h on one thread: g, o as float4 rows; normals of rows [0, rows) against all n points
extern "C" long long baseline_normals(const float* g, const float* o, long long n, long long rows, float radius, int min_neighbours, float* out,
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
    const float scale = std::ldexp(1.0f, 20 - e), r2 = radius * radius;
    long long without = 0;
    for (long long i = 0; i < rows; ++i) {
        const float qx = g[4 * i], qy = g[4 * i + 1], qz = g[4 * i + 2];
        const long long cx = (long long)std::floor(qx / cell), cy = (long long)std::floor(qy / cell), cz = (long long)std::floor(qz / cell);
        long long m[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
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
                        if (!(d2 <= r2)) continue;
                        const long long ix = (int)std::rint(dx * scale), iy = (int)std::rint(dy * scale), iz = (int)std::rint(dz * scale);
                        m[0] += 1, m[1] += ix, m[2] += iy, m[3] += iz, m[4] += ix * ix, m[5] += ix * iy, m[6] += ix * iz, m[7] += iy * iy, m[8] += iy * iz, m[9] += iz * iz;
                    }
                }
        if (!dmsa::dense_normal_from_moments(m, o[4 * i] - qx, o[4 * i + 1] - qy, o[4 * i + 2] - qz, min_neighbours, out + 4 * i)) ++without;
    }
    seconds[0] = std::chrono::duration<double>(t1 - t0).count(), seconds[1] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    return without;
}
"""


def build_baseline(tmp):
    src, lib = os.path.join(tmp, "normals_baseline.cpp"), os.path.join(tmp, "libnormals_baseline.so")
    with open(src, "w") as f:
        f.write(BASELINE_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "dmsa_lidar_slam_amd", "csrc"), "-o", lib, src])
    L = C.CDLL(lib)
    L.baseline_normals.restype = C.c_longlong
    L.baseline_normals.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_longlong, C.c_longlong, C.c_float, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_double)]
    return L


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def spread(runs):
    return {"median_s": round(statistics.median(runs), 4), "min_s": round(min(runs), 4), "max_s": round(max(runs), 4), "repeats": len(runs)}


def pmc_of(directory, kernel="k_neighbour_moments"):
    """Counter sums over the dispatches of `kernel` from the *counter_collection.csv of a rocprofv3 --pmc run."""
    sums, dispatches = {}, set()
    for path in glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if kernel in row.get("Kernel_Name", ""):
                sums[row["Counter_Name"]] = sums.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
                dispatches.add(row.get("Dispatch_Id"))
    if not sums:
        raise SystemExit(f"no counters of {kernel} under {directory}")
    return {"kernel": kernel, "dispatches": len(dispatches), "counters": sums}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--min-range", type=float, default=0.5)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--min-neighbours", type=int, default=5)
    ap.add_argument("--baseline-rows", type=int, default=300000, help="rows the one-thread host figure computes (against all retained points)")
    ap.add_argument("--keep", help="write the dump and the poses here and leave them (for the profiler runs)")
    ap.add_argument("--out", help="JSON file the figures are written to (merged into what it already holds)")
    ap.add_argument("--kernel-stats", help="directory of a rocprofv3 --kernel-trace --stats run of examples/dense_cloud_from_raw with a radius")
    ap.add_argument("--pmc", help="directory of a rocprofv3 --pmc run of the same command (a run of its own)")
    a = ap.parse_args()
    result = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    if a.kernel_stats:
        ks = dct.kernel_stats(a.kernel_stats)
        normals = {k: v for k, v in ks["kernels_us"].items() if "normals" in k or "neighbour_moments" in k or "normal_rows" in k or "sort" in k.lower() or "onesweep" in k.lower()}
        total = sum(v["total_us"] for v in normals.values())
        ks["normals_kernels_us"] = normals
        ks["normals_kernel_s"] = round(total / 1e6, 4)
        ks["share_of_normals_kernel_time"] = {k: round(v["total_us"] / total, 4) for k, v in sorted(normals.items(), key=lambda kv: -kv[1]["total_us"])} if total else {}
        result["profile"] = ks
    elif a.pmc:
        result["pmc"] = pmc_of(a.pmc)
    else:
        from dmsa_lidar_slam_amd import raw_sequence as rs
        from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator

        with tempfile.TemporaryDirectory() as tmp:
            work = a.keep or tmp
            os.makedirs(work, exist_ok=True)
            dump, poses, _ = dct.make_sequence(work, a.messages, a.points)
            dc = DenseCloudCreator.from_tum_file(poses, DenseCloudConfig(minRange=a.min_range, voxelSize=a.voxel), retain=True)
            fill_s, _ = timed(lambda: [dc.add_pointcloud2(msg, "ouster", download=False) for kind, msg in rs.RawReader(dump) if kind == "pointcloud2"])
            n = dc.retained_count()
            other = a.radius * 1.25  # the grid of another radius: the timed call then builds its own

            def one_run(path):
                dc.neighbour_moments(other, 0, 1)
                t_compute, (_, without) = timed(lambda: dc.compute_normals(a.radius, a.min_neighbours, download=False))
                t_save, (points, size) = timed(lambda: dc.save_pcd_normals(path))
                assert points == n
                return t_compute, t_save, without, size

            f_local = os.path.join(tmp, "normals.pcd")
            figures = {}
            for tag, path in (("dev_null", "/dev/null"), ("local_file", f_local)):
                one_run(path)  # warm-up: buffers, code objects, page cache
                runs = [one_run(path) for _ in range(a.repeats)]
                figures[tag] = {"compute_normals": spread([r[0] for r in runs]), "save_pcd_normals": spread([r[1] for r in runs]),
                                "end_to_end": spread([r[0] + r[1] for r in runs]), "without_normal": runs[0][2], "file_bytes": runs[0][3]}
                figures[tag]["rows_per_s"] = round(n / figures[tag]["end_to_end"]["median_s"])
            # the one-thread host figure on the same retained points
            g, o = dc.retained()
            normals, _ = dc.compute_normals(a.radius, a.min_neighbours)
            moments_head = dc.neighbour_moments(a.radius, 0, min(n, 100000))
            dc.close()
            rows = min(a.baseline_rows, n)
            L = build_baseline(tmp)
            out = np.zeros((rows, 4), np.float32)
            fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
            sec = (C.c_double * 2)()
            L.baseline_normals(fp(g), fp(o), n, rows, a.radius, a.min_neighbours, fp(out), sec)
            grid_s, rows_s = float(sec[0]), float(sec[1])
            result.update({
                "workload": {"messages": a.messages, "points_per_message": a.points, "voxel_size": a.voxel, "min_range": a.min_range, "radius": a.radius,
                             "min_neighbours": a.min_neighbours, "retained_rows": n, "fill_store_s": round(fill_s, 3),
                             "neighbours_per_row_mean_first_100k": round(float(moments_head[:, 0].mean()), 2), "neighbours_per_row_max_first_100k": int(moments_head[:, 0].max())},
                "device": figures,
                "host_one_thread": {"rows": rows, "grid_s": round(grid_s, 3), "rows_s": round(rows_s, 3), "rows_per_s": round(rows / rows_s),
                                    "scaled_to_all_rows_s": round(grid_s + rows_s * n / rows, 1),
                                    "normals_equal_device_bits": bool(np.array_equal(out.view(np.uint32), normals[:rows].view(np.uint32)))},
            })
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
