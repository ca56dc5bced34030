"""Time of the dense cloud's occupancy map (include/dmsa_dense_occupancy.h) on the workload of profiles/r09_dense_cloud.json: 200 Ouster messages
of 131 072 points, voxel 0.1 m; the default config (cells of 0.2 m, max_length 30 m).

    python scripts/dense_occupancy_time.py --out profiles/r28_dense_occupancy.json
    rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- python scripts/dense_occupancy_time.py --kernels-only
    python scripts/dense_occupancy_time.py --trace DIR --out profiles/r28_dense_occupancy.json

End to end is dmsa_dense_cloud_build_occupancy on a store whose search grid has the cells' edge already (count_passes ran before it: the carve
stage comes first in every pipeline): the table cleared, k_occupancy_walk, the small read, the listing (flags, scan, compaction, 64-bit sort,
states) and the final read; median of 5 after a warm-up.  The statistics must be the same integers in every run.  Beside it: the slice of
0.2 .. 1.5 m, and the two writers to /dev/null.
The kernel figures come from ONE rocprofv3 --kernel-trace run of --kernels-only (no counters are collected in it): k_occupancy_walk against
k_carve_passes of the same process, which walks the same cells with a probe per cell and no insert -- the floor the walk can approach.
The host figure is ONE thread doing M2-M3 through the header the device kernels compile (csrc/dense_carve_walk.h) into a std::unordered_map
-- a small C++ helper this script builds -- for the shortest --baseline-fraction of the rays.  That is the subset the device walks when
max_length is the longest of these rays' lengths, so the device's listing for exactly these rays exists and is compared cell for cell.  The
host time is then SCALED to all rays by the number of traversed cells.  No ratio is fixed in advance."""
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

SLAB = (0.2, 1.5)

BASELINE_SRC = r"""
#include <chrono>
#include <cstdint>
#include <unordered_map>
#include "dense_carve_walk.h"
using namespace dmsa;
struct Counts { uint32_t hits = 0, passes = 0; };
static std::unordered_map<uint64_t, Counts> table;
// M2-M3 of dmsa_dense_occupancy.h on one thread: g and o as float4 rows; returns the cells of the map
extern "C" long long baseline_occupancy(const float* g, const float* o, long long n, float cell_size, float max_length, long long* sums /* skipped, cells, outside */,
                                        double* seconds) {
    const auto t0 = std::chrono::steady_clock::now();
    const double c = (double)cell_size;
    table.clear();
    sums[0] = sums[1] = sums[2] = 0;
    for (long long r = 0; r < n; ++r) {
        const float* e = g + 4 * r;
        const float* s = o + 4 * r;
        const CarveRay ray = carve_ray(s[0], s[1], s[2], e[0], e[1], e[2]);
        CarveWalk w;
        if (carve_ray_skipped(ray, max_length) || !carve_walk_begin(c, s[0], s[1], s[2], e[0], e[1], e[2], &w)) {
            ++sums[0];
            continue;
        }
        for (int32_t step = 0; step <= kCarveMaxSteps; ++step) {
            ++sums[1];
            const bool last = !(w.lx > 0 || w.ly > 0 || w.lz > 0);
            if (carve_cell_holds_rows(w)) {
                Counts& k = table[(uint64_t)(w.cx + 1048576) << 42 | (uint64_t)(w.cy + 1048576) << 21 | (uint64_t)(w.cz + 1048576)];
                if (last) ++k.hits; else ++k.passes;
            } else {
                ++sums[2];
            }
            if (!carve_walk_step(&w)) break;
        }
    }
    seconds[0] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return (long long)table.size();
}
extern "C" void baseline_cells(uint64_t* key, uint32_t* hits, uint32_t* passes) {
    long long i = 0;
    for (const auto& kv : table) key[i] = kv.first, hits[i] = kv.second.hits, passes[i] = kv.second.passes, ++i;
}
"""


def build_baseline(tmp):
    src, lib = os.path.join(tmp, "occupancy_baseline.cpp"), os.path.join(tmp, "liboccupancy_baseline.so")
    with open(src, "w") as f:
        f.write(BASELINE_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "dmsa_lidar_slam_amd", "csrc"), "-o", lib, src])
    L = C.CDLL(lib)
    L.baseline_occupancy.restype = C.c_longlong
    L.baseline_occupancy.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_longlong, C.c_float, C.c_float, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    L.baseline_cells.restype = None
    L.baseline_cells.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    return L


def run_baseline(L, g, o, cfg):
    """(keys ascending, hits, passes, (skipped, cells, outside), seconds) of M2-M3 with this config on one host thread."""
    g, o = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(o, np.float32)
    sums, sec = (C.c_longlong * 3)(), (C.c_double * 1)()
    c = cfg.to_c()
    m = L.baseline_occupancy(g.ctypes.data_as(C.POINTER(C.c_float)), o.ctypes.data_as(C.POINTER(C.c_float)), g.shape[0], c.cell_size, c.max_length, sums, sec)
    key, hits, passes = np.zeros(m, np.uint64), np.zeros(m, np.uint32), np.zeros(m, np.uint32)
    L.baseline_cells(key.ctypes.data_as(C.POINTER(C.c_uint64)), hits.ctypes.data_as(C.POINTER(C.c_uint32)), passes.ctypes.data_as(C.POINTER(C.c_uint32)))
    order = np.argsort(key)
    return key[order], hits[order], passes[order], tuple(int(v) for v in sums), float(sec[0])


def trace_figures(directory):
    """Durations [ms] per kernel from the *kernel_trace.csv of a rocprofv3 --kernel-trace run; the first dispatch of each (the warm-up) left out."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6) for r in csv.DictReader(open(path))]
    rows.sort()
    out = {}
    for name in ("k_occupancy_walk", "k_carve_passes", "k_occupancy_clear", "k_occupancy_flags", "k_occupancy_compact", "k_occupancy_states", "k_occupancy_rows",
                 "k_occupancy_extent", "k_occupancy_columns", "k_occupancy_pixels"):
        ms = [d for _, kernel, d in rows if name + "(" in kernel][1:]
        if ms:
            out[name + "_ms"] = {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "dispatches": len(ms)}
    if "k_occupancy_walk_ms" in out and "k_carve_passes_ms" in out:
        out["walk_over_carve_passes"] = round(out["k_occupancy_walk_ms"]["median"] / out["k_carve_passes_ms"]["median"], 2)
    return out


def key_of(cells):
    c = cells.astype(np.int64) + (1 << 20)
    return ((c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--min-range", type=float, default=0.5)
    ap.add_argument("--baseline-fraction", type=float, default=0.02, help="the one-thread host figure walks this fraction of the rays, the shortest ones")
    ap.add_argument("--kernels-only", action="store_true", help="the device work alone, for a profiler run")
    ap.add_argument("--trace", help="the output directory of a rocprofv3 --kernel-trace run of --kernels-only: its per-kernel figures are merged into --out")
    ap.add_argument("--out", help="JSON file the figures are written to (merged into what it already holds)")
    a = ap.parse_args()
    result = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    equal = True
    if a.trace:
        result["kernels_from_one_kernel_trace_run"] = trace_figures(a.trace)
    else:
        from dmsa_lidar_slam_amd import raw_sequence as rs
        from dmsa_lidar_slam_amd.dense_cloud import DenseCarveConfig, DenseCloudConfig, DenseCloudCreator, DenseOccupancyConfig

        cfg = DenseOccupancyConfig()
        with tempfile.TemporaryDirectory() as tmp:
            dump, poses, _ = dct.make_sequence(tmp, a.messages, a.points)
            dc = DenseCloudCreator.from_tum_file(poses, DenseCloudConfig(minRange=a.min_range, voxelSize=a.voxel), retain=True)
            for kind, msg in rs.RawReader(dump):
                if kind == "pointcloud2":
                    dc.add_pointcloud2(msg, "ouster", download=False)
            n = dc.retained_count()
            carve = DenseCarveConfig()
            dc.count_passes(carve)  # warm-up, and the grid at the cells' edge
            t_carve = spread([timed(lambda: dc.count_passes(carve))[0] for _ in range(a.repeats)])
            _, stats = timed(lambda: dc.build_occupancy(cfg))  # warm-up: code objects, buffers
            runs = [timed(lambda: dc.build_occupancy(cfg)) for _ in range(a.repeats)]
            assert all(r[1] == stats for r in runs)  # the same integers every run
            dc.occupancy_slice(*SLAB)
            slices = [timed(lambda: dc.occupancy_slice(*SLAB)) for _ in range(a.repeats)]
            info = slices[0][1][0]
            dc.save_pcd_occupancy("/dev/null", 0)
            saves = [timed(lambda: dc.save_pcd_occupancy("/dev/null", 0)) for _ in range(a.repeats)]
            maps = [timed(lambda: dc.save_occupancy_map("/dev/null", "/dev/null", *SLAB)) for _ in range(a.repeats)]
            figures = {"build_occupancy": spread([r[0] for r in runs]), "count_passes_same_process": t_carve, "occupancy_slice_with_download": spread([r[0] for r in slices]),
                       "save_pcd_occupancy": spread([r[0] for r in saves]), "save_occupancy_map": spread([r[0] for r in maps]),
                       "voxel_file_bytes": 24 * stats["cells"], "rays_per_s": round(n / statistics.median([r[0] for r in runs]))}
            print("device:", json.dumps(figures), json.dumps(stats), flush=True)
            result.update({"workload": {"messages": a.messages, "points_per_message": a.points, "voxel_size": a.voxel, "min_range": a.min_range, "retained_rows": n,
                                        "config": {k: getattr(cfg, k) for k in ("cell_size", "max_length", "min_hits", "min_passes", "occ_num", "occ_den")}, "slab_m": list(SLAB)},
                           "counts": stats, "slice": info, "device": figures})
            if not a.kernels_only:
                g, o = dc.retained()
                d = g[:, :3] - o[:, :3]
                length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
                assert length.dtype == np.float32
                at = int(a.baseline_fraction * length.shape[0])
                limit = float(np.partition(length, at)[at])
                short = DenseOccupancyConfig(max_length=limit)
                short_stats = dc.build_occupancy(short)
                cells, hits, passes, _ = dc.occupancy_cells()
                assert short_stats["rays_walked"] == int((length <= np.float32(limit)).sum()) > 0
                print(f"host baseline: {short_stats['rays_walked']} rays with L <= {limit:.4f} m", flush=True)
                key_h, hits_h, passes_h, sums, rays_s = run_baseline(build_baseline(tmp), g, o, short)
                equal = (np.array_equal(key_h, key_of(cells)) and np.array_equal(hits_h, hits) and np.array_equal(passes_h, passes)
                         and sums == (short_stats["rays_skipped"], short_stats["cells_traversed"], short_stats["cells_out_of_range"]))
                print(f"host baseline: cells host {key_h.shape[0]}, device {cells.shape[0]}; sums (skipped, cells, outside) host {sums}; equal: {equal}", flush=True)
                result["host_one_thread"] = {"subset": f"the rays with L <= {limit:.6g} m (the shortest {a.baseline_fraction:g} of all)", "rays_walked": short_stats["rays_walked"],
                                             "cells_traversed": sums[1], "map_cells": int(key_h.shape[0]), "rays_s": round(rays_s, 3),
                                             "scaled_to_all_rays_by_cells_s": round(rays_s * stats["cells_traversed"] / max(sums[1], 1), 1),
                                             "counts_equal_device": bool(equal)}
            dc.close()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    assert equal, "the host baseline's counts differ from the device's"


if __name__ == "__main__":
    main()
