"""Time of the dense cloud's ray carving (include/dmsa_dense_carve.h) on the workload of profiles/r09_dense_cloud.json: 200 Ouster messages of
131 072 points, voxel 0.1 m; the default carve config.

    python scripts/dense_carve_time.py --out profiles/r13_dense_carve.json

End to end is the time from "the retained store is complete" to "the x y z file of the carved store is written":
dmsa_dense_cloud_count_passes (cell keys, sort, cell table, k_carve_passes, the flags and their scan), dmsa_dense_cloud_remove_transients and
dmsa_dense_cloud_save_pcd_retained to /dev/null, each ending in a host wait; median of 5 after a warm-up.  remove_transients changes the store,
so every run fills a fresh object from the same dump (not timed).  The statistics must be the same integers in every run.
The host figure is ONE thread doing T2-T6 over a hash grid (std::unordered_map of cell -> rows) through the header the device kernels compile
(csrc/dense_carve_walk.h) -- a small C++ helper this script builds -- for a SUBSET of the rays against the full store: the shortest
--baseline-fraction of them.  That is the subset the device walks when max_length is set to the longest of these rays' lengths, so the device's
`passes` for exactly these rays exist and are compared bit for bit.  The host time is then SCALED to all rays by the number of traversed cells
and, beside it, by the number of pair tests (short rays are cheaper than the average ray: a scaling per ray would flatter the host).  No ratio is fixed in advance."""
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
#include <cstdint>
#include <unordered_map>
#include <vector>
#include "dense_carve_walk.h"
using namespace dmsa;
// T2-T6 of dmsa_dense_carve.h on one thread: g and o as float4 rows; passes[j] += rays among all n that see through row j
extern "C" void baseline_carve(const float* g, const float* o, long long n, float cell_size, float rho, float tan_half_angle, float end_margin, float start_margin,
                               float max_length, uint32_t* passes, long long* sums /* skipped, cells, pairs, seen */, double* seconds /* grid, rays */) {
    const auto t0 = std::chrono::steady_clock::now();
    const double c = (double)cell_size;
    auto key_of = [](long long x, long long y, long long z) { return (uint64_t)(x + 1048576) << 42 | (uint64_t)(y + 1048576) << 21 | (uint64_t)(z + 1048576); };
    std::unordered_map<uint64_t, std::vector<uint32_t>> grid;
    grid.reserve((size_t)n / 4);
    for (long long i = 0; i < n; ++i)
        grid[key_of((long long)std::floor(g[4 * i] / c), (long long)std::floor(g[4 * i + 1] / c), (long long)std::floor(g[4 * i + 2] / c))].push_back((uint32_t)i);
    const auto t1 = std::chrono::steady_clock::now();
    const CarvePair pair = carve_pair(rho, tan_half_angle, end_margin, start_margin);
    sums[0] = sums[1] = sums[2] = sums[3] = 0;
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
            if (carve_cell_holds_rows(w)) {
                const auto it = grid.find(key_of(w.cx, w.cy, w.cz));
                if (it != grid.end())
                    for (const uint32_t j : it->second) {
                        if ((long long)j == r) continue;
                        ++sums[2];
                        if (carve_sees_through(ray, pair, e[0], e[1], e[2], g[4 * j], g[4 * j + 1], g[4 * j + 2])) ++sums[3], ++passes[j];
                    }
            }
            if (!carve_walk_step(&w)) break;
        }
    }
    seconds[0] = std::chrono::duration<double>(t1 - t0).count(), seconds[1] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
}
"""


def build_baseline(tmp):
    src, lib = os.path.join(tmp, "carve_baseline.cpp"), os.path.join(tmp, "libcarve_baseline.so")
    with open(src, "w") as f:
        f.write(BASELINE_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "dmsa_lidar_slam_amd", "csrc"), "-o", lib, src])
    L = C.CDLL(lib)
    L.baseline_carve.restype = None
    L.baseline_carve.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_longlong] + [C.c_float] * 6 + [C.POINTER(C.c_uint32), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    return L


def run_baseline(L, g, o, cfg):
    """(passes, (skipped, cells, pairs, seen), seconds for the grid, seconds for the rays) of T2-T6 with this config on one host thread."""
    g, o = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(o, np.float32)
    passes, sums, sec = np.zeros(g.shape[0], np.uint32), (C.c_longlong * 4)(), (C.c_double * 2)()
    c = cfg.to_c()
    L.baseline_carve(g.ctypes.data_as(C.POINTER(C.c_float)), o.ctypes.data_as(C.POINTER(C.c_float)), g.shape[0], c.cell_size, c.rho, c.tan_half_angle, c.end_margin,
                     c.start_margin, c.max_length, passes.ctypes.data_as(C.POINTER(C.c_uint32)), sums, sec)
    return passes, tuple(int(v) for v in sums), float(sec[0]), float(sec[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--min-range", type=float, default=0.5)
    ap.add_argument("--baseline-fraction", type=float, default=0.02,
                    help="the one-thread host figure walks this fraction of the rays, the shortest ones (against all retained points)")
    ap.add_argument("--baseline-only", action="store_true", help="keep the device figures --out already holds and redo the host figure only")
    ap.add_argument("--out", help="JSON file the figures are written to (merged into what it already holds)")
    a = ap.parse_args()
    result = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    from dmsa_lidar_slam_amd import raw_sequence as rs
    from dmsa_lidar_slam_amd.dense_cloud import DenseCarveConfig, DenseCloudConfig, DenseCloudCreator

    cfg = DenseCarveConfig()
    with tempfile.TemporaryDirectory() as tmp:
        dump, poses, _ = dct.make_sequence(tmp, a.messages, a.points)

        def filled():
            dc = DenseCloudCreator.from_tum_file(poses, DenseCloudConfig(minRange=a.min_range, voxelSize=a.voxel), retain=True)
            sec, _ = timed(lambda: [dc.add_pointcloud2(msg, "ouster", download=False) for kind, msg in rs.RawReader(dump) if kind == "pointcloud2"])
            return dc, sec

        def one_run(path):
            dc, fill_s = filled()
            n = dc.retained_count()
            t_count, stats = timed(lambda: dc.count_passes(cfg))
            t_remove, left = timed(dc.remove_transients)
            t_save, (points, size) = timed(lambda: dc.save_pcd_retained(path))
            dc.close()
            assert points == left == stats["kept"] and stats["rows"] == n
            print(f"run: count_passes {t_count:.3f} s  remove_transients {t_remove:.3f} s  save {t_save:.3f} s  (fill {fill_s:.1f} s)", flush=True)
            return t_count, t_remove, t_save, stats, size, fill_s

        if a.baseline_only:
            figures, stats, fill_s = result["device"], result["counts"], result["workload"]["fill_store_s"]
        else:
            one_run("/dev/null")  # warm-up: code objects
            runs = [one_run("/dev/null") for _ in range(a.repeats)]
            figures = {"count_passes": spread([r[0] for r in runs]), "remove_transients": spread([r[1] for r in runs]), "save_pcd_retained": spread([r[2] for r in runs]),
                       "end_to_end": spread([r[0] + r[1] + r[2] for r in runs]), "file_bytes": runs[0][4]}
            figures["rays_per_s"] = round(runs[0][3]["rows"] / figures["end_to_end"]["median_s"])
            assert all(r[3] == runs[0][3] for r in runs)  # the same integers every run
            stats, fill_s = runs[0][3], runs[0][5]
        # the one-thread host figure: the shortest --baseline-fraction of the rays against the full store.  T2's length in float32, operation for
        # operation, so that `L <= max_length` selects the same rays here, on the device and in the helper
        dc, _ = filled()
        g, o = dc.retained()
        assert g.shape[0] == stats["rows"]
        d = g[:, :3] - o[:, :3]
        length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        assert length.dtype == np.float32
        limit = float(np.partition(length, int(a.baseline_fraction * length.shape[0]))[int(a.baseline_fraction * length.shape[0])])
        short = DenseCarveConfig(max_length=limit)
        short_stats, device_passes = dc.count_passes(short, download=True)
        dc.close()
        assert short_stats["rays_walked"] == int((length <= np.float32(limit)).sum()) > 0
        print(f"host baseline: {short_stats['rays_walked']} rays with L <= {limit:.4f} m", flush=True)
        passes, sums, grid_s, rays_s = run_baseline(build_baseline(tmp), g, o, short)
        print(f"host baseline: {int((passes != device_passes).sum())} rows differ from the device; sums (skipped, cells, pairs, seen) host {sums}, device "
              f"{tuple(short_stats[k] for k in ('rays_skipped', 'cells_traversed', 'pair_tests', 'seen_through'))}", flush=True)
        equal = bool(np.array_equal(passes, device_passes)) and sums ==(short_stats["rays_skipped"], short_stats["cells_traversed"], short_stats["pair_tests"], short_stats["seen_through"])
        result.update({
            "workload": {"messages": a.messages, "points_per_message": a.points, "voxel_size": a.voxel, "min_range": a.min_range, "retained_rows": stats["rows"],
                         "fill_store_s": round(fill_s, 3), "config": {k: getattr(cfg, k) for k in ("cell_size", "rho", "tan_half_angle", "end_margin", "start_margin", "max_length", "min_passes")}},
            "counts": stats,
            "device": figures,
            "host_one_thread": {"subset": f"the rays with L <= {limit:.6g} m (the shortest {a.baseline_fraction:g} of all) against all retained rows",
                                "rays_walked": short_stats["rays_walked"],
                                "cells_traversed": sums[1], "pair_tests": sums[2], "seen_through": sums[3], "grid_s": round(grid_s, 3), "rays_s": round(rays_s, 3),
                                "scaled_to_all_rays_by_cells_s": round(grid_s + rays_s * stats["cells_traversed"] / max(sums[1], 1), 1),
                                "scaled_to_all_rays_by_pair_tests_s": round(grid_s + rays_s * stats["pair_tests"] / max(sums[2], 1), 1),
                                "passes_and_sums_equal_device": equal},
        })
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    assert equal, "the host baseline's passes differ from the device's"


if __name__ == "__main__":
    main()
