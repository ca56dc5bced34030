"""Time of the alignment of the dense cloud's reference by ICP (include/dmsa_dense_align.h) on the workload of profiles/r09_dense_cloud.json:
200 Ouster messages of 131 072 points, voxel 0.1 m.  The reference is the retained store itself, every row displaced by a fixed
pseudo-random offset below half a voxel per axis and then moved by the inverse of a known small rigid motion (0.5 degrees, 0.05 m), so the
alignment has that motion to find.  max_distance 0.3 m and again 1.0 m.

    python scripts/dense_align_time.py --out profiles/r22_dense_align.json
    rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- python scripts/dense_align_time.py --kernels-only
    python scripts/dense_align_time.py --trace DIR --out profiles/r22_dense_align.json

The first form times in ONE process, each figure a median of 5 after a warm-up and each ending in a host wait, the parts an iteration is made
of, through the calls that are those parts: dmsa_dense_cloud_set_reference with a transform (the upload and the transform: the loop itself
uploads once), dmsa_dense_cloud_align_sums right after it (the reference's grid rebuilt, k_nearest_across, both sums kernels, the copy
back), the same call again (the grid kept: the difference is the grid build), dmsa_dense_align_solve on the host, and the yardstick
dmsa_dense_cloud_compare at the same max_distance (both directions, the grids kept: half of it is one direction).  Then
dmsa_dense_cloud_align_reference end to end and its time per iteration.  ONE host thread adds the same 25 sums over the same pairs (a small
C++ helper this script builds, 128-bit accumulators, ALL rows, not a sample) and must give the device's 25 words.
The second form is the device work alone, for a profiler run of its own; the third reads that run's kernel trace: per dispatch of
k_nearest_across, k_align_pair_sums, k_compare_quantise_sum, k_reference_transform and k_reference_cell_keys, medians.
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
// A2 of dmsa_dense_align.h on one thread: the pairs (p[i], g[index[i]]) with index[i] >= 0; words = the 25 sums, lo and hi recombined and split again
extern "C" void baseline_pair_sums(const float* p, const float* g, const int* index, long long n, float scale_c, long long* words, double* seconds) {
    const auto t0 = std::chrono::steady_clock::now();
    __int128 cross[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    long long pairs = 0, sp[3] = {0, 0, 0}, sg[3] = {0, 0, 0};
    for (long long i = 0; i < n; ++i) {
        if (index[i] < 0) continue;
        long long P[3], G[3];
        for (int a = 0; a < 3; ++a) P[a] = (long long)std::rint(p[3 * i + a] * scale_c), G[a] = (long long)std::rint(g[3 * (long long)index[i] + a] * scale_c);
        ++pairs;
        for (int a = 0; a < 3; ++a) {
            sp[a] += P[a], sg[a] += G[a];
            for (int b = 0; b < 3; ++b) cross[3 * a + b] += (__int128)(P[a] * G[b]);
        }
    }
    words[0] = pairs;
    for (int a = 0; a < 3; ++a) words[1 + a] = sp[a], words[4 + a] = sg[a];
    for (int k = 0; k < 9; ++k) words[7 + 2 * k] = (long long)(cross[k] & 0xFFFFFFFF), words[8 + 2 * k] = (long long)(cross[k] >> 32);
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
"""


def build_baseline(tmp):
    src, lib = os.path.join(tmp, "align_baseline.cpp"), os.path.join(tmp, "libalign_baseline.so")
    with open(src, "w") as f:
        f.write(BASELINE_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    L.baseline_pair_sums.restype = None
    L.baseline_pair_sums.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_longlong, C.c_float, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    return L


def rigid(deg, axis, t):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.radians(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.concatenate([np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K), np.asarray(t, np.float64).reshape(3, 1)], axis=1)


def trace_figures(directory):
    """Durations [ms] per dispatch from the *kernel_trace.csv of a rocprofv3 --kernel-trace run."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6) for r in csv.DictReader(open(path))]
    out = {}
    for name in ("k_nearest_across", "k_align_pair_sums", "k_compare_quantise_sum", "k_reference_transform", "k_reference_cell_keys"):
        ms = [t for kernel, t in rows if name in kernel]
        if ms:
            out[name + "_ms"] = {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "dispatches": len(ms)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--min-range", type=float, default=0.5)
    ap.add_argument("--degrees", type=float, default=0.5)
    ap.add_argument("--metres", type=float, default=0.05)
    ap.add_argument("--kernels-only", action="store_true", help="the device work alone, for a profiler run")
    ap.add_argument("--trace", help="the output directory of a rocprofv3 --kernel-trace run of --kernels-only: its per-kernel figures are merged into --out")
    ap.add_argument("--out", help="JSON file the figures are written to (merged into what it already holds)")
    a = ap.parse_args()
    result = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    if a.trace:
        result["kernels_from_one_kernel_trace_run"] = trace_figures(a.trace)
    else:
        from dmsa_lidar_slam_amd import raw_sequence as rs
        from dmsa_lidar_slam_amd import _capi as capi
        from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator, align_solve, align_sum_words

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
            start = np.eye(3, 4)
            dc.set_reference(ref, start)  # warm-up
            figures = {}
            for reach in REACHES:
                dc.compare(reach, min(0.1, reach))  # warm-up: the store's grid at this edge
                transform, rebuilt, kept = [], [], []
                for _ in range(a.repeats):
                    transform.append(timed(lambda: dc.set_reference(ref, start))[0])
                    t, sums = timed(lambda: dc.align_sums(reach))
                    rebuilt.append(t)
                    t, again = timed(lambda: dc.align_sums(reach))
                    kept.append(t)
                    assert again == sums  # the same integers every run
                solve = [timed(lambda: align_solve(sums, scale_c))[0] for _ in range(a.repeats)]
                compare = [timed(lambda: dc.compare(reach, min(0.1, reach)))[0] for _ in range(a.repeats)]
                dc.align_reference(ref, max_distance=reach, max_iterations=2)  # warm-up
                runs = [timed(lambda: dc.align_reference(ref, max_distance=reach)) for _ in range(a.repeats)]
                out = runs[0][1]
                assert all(r[1]["transform"].tobytes() == out["transform"].tobytes() and r[1]["history"] == out["history"] for r in runs)  # the same bytes every run
                per_iteration = [r[0] / out["iterations"] for r in runs]
                figures[f"max_distance_{reach:g}"] = {
                    "set_reference_upload_and_transform": spread(transform), "align_sums_reference_grid_rebuilt": spread(rebuilt), "align_sums_grids_kept": spread(kept),
                    "reference_grid_build_by_difference_s": round(statistics.median(rebuilt) - statistics.median(kept), 4), "align_solve_host": spread(solve),
                    "compare_both_directions_grids_kept": spread(compare), "one_direction_of_compare_s": round(statistics.median(compare) / 2, 4),
                    "align_reference": spread([r[0] for r in runs]), "align_reference_per_iteration": spread(per_iteration), "iterations": out["iterations"], "stop": out["stop"],
                    "pairs_first_iteration": out["history"][0]["matched"], "rms_first_m": out["history"][0]["rms_m"], "rms_last_m": out["history"][-1]["rms_m"],
                    "largest_entry_error_against_the_applied_motion": float(np.abs(out["transform"] - motion).max())}
            result.update({"workload": {"messages": a.messages, "points_per_message": a.points, "voxel_size": a.voxel, "min_range": a.min_range, "retained_rows": n,
                                        "reference_rows": n, "degrees": a.degrees, "metres": a.metres,
                                        "reference": "the store, every row displaced by a fixed pseudo-random offset below half a voxel per axis, then moved by the inverse of the motion"},
                           "device": figures})
            if not a.kernels_only:
                L = build_baseline(tmp)
                host = {}
                for reach in REACHES:
                    dc.set_reference(ref, start)
                    words = align_sum_words(dc.align_sums(reach))
                    _, index = dc.nearest_in_store(reach)
                    p, _ = dc.reference()
                    got, sec = (C.c_longlong * 25)(), C.c_double(0)
                    fp = lambda arr: np.ascontiguousarray(arr, np.float32).ctypes.data_as(C.POINTER(C.c_float))
                    store = np.ascontiguousarray(g[:, :3], np.float32)
                    L.baseline_pair_sums(fp(p), fp(store), np.ascontiguousarray(index, np.int32).ctypes.data_as(C.POINTER(C.c_int)), n, scale_c, got, C.byref(sec))
                    host[f"max_distance_{reach:g}"] = {"rows": n, "pair_sums_one_thread_all_rows_s": round(sec.value, 4), "words_equal_device": list(got) == words}
                    assert host[f"max_distance_{reach:g}"]["words_equal_device"]
                result["host_one_thread_pair_sums_given_the_pairs"] = host
            dc.close()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
