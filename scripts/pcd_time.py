"""Time of the PointCloud.pcd export (include/dmsa_wire_formats.h) at the size of the config-4 map: 249 keyframes, ~2.5 M points
with normals, resident in HBM.

    python scripts/pcd_time.py --out profiles/r08_pcd_export.json          device path vs the host baseline, to /dev/null and to a local file
    rocprofv3 --kernel-trace --memory-copy-trace --stats -d DIR -o pcd -- python scripts/pcd_time.py --saves-only 5
    python scripts/pcd_time.py --kernel-stats DIR --out profiles/r08_pcd_export.json     adds kernel-only time and the copy-back share of that run

The baseline is one host thread doing snprintf("%.8g") per value into a buffer plus fwrite -- a small C++ helper this script builds.  It stands in
for PCL's ostream writer (which is certainly no faster) on the SAME machine; no threshold is fixed in advance."""
import argparse
import ctypes as C
import glob
import json
import os
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASELINE_SRC = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
// one thread: seven "%.8g" per row into a buffer, fwrite per 65536 rows
extern "C" long long baseline_save(const char* path, const char* header, const float* xyz, const float* nrm, long long n) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return -1;
    long long bytes = std::fputs(header, f) >= 0 ? 0 : -1;
    for (const char* h = header; *h; ++h) ++bytes;
    std::vector<char> buf(65536 * 106 + 1);
    for (long long at = 0; at < n; at += 65536) {
        char* p = buf.data();
        const long long end = at + 65536 < n ? at + 65536 : n;
        for (long long i = at; i < end; ++i)
            p += std::snprintf(p, 106, "%.8g %.8g %.8g %.8g %.8g %.8g 0\n", (double)xyz[4 * i], (double)xyz[4 * i + 1], (double)xyz[4 * i + 2], (double)nrm[4 * i],
                               (double)nrm[4 * i + 1], (double)nrm[4 * i + 2]);
        if (std::fwrite(buf.data(), 1, (size_t)(p - buf.data()), f) != (size_t)(p - buf.data())) return -2;
        bytes += p - buf.data();
    }
    return std::fclose(f) == 0 ? bytes : -3;
}
"""


def build_baseline(tmp):
    src, lib = os.path.join(tmp, "pcd_baseline.cpp"), os.path.join(tmp, "libpcd_baseline.so")
    with open(src, "w") as f:
        f.write(BASELINE_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    L.baseline_save.restype = C.c_longlong
    L.baseline_save.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_longlong]
    return L


def resident_map(frames):
    from dmsa_lidar_slam_amd import synth
    from dmsa_lidar_slam_amd.api import DmsaOptimizer

    prob = synth.keyframe_problem(seed=1, frames=frames, arc=2 * np.pi * frames / 256.0)  # the map of bench.py --workload keyframes
    opt = DmsaOptimizer(device=0)
    opt.upload(prob)
    opt.poseTables(opt.getPoseParameters(), download=False)
    opt.updateGlobalPoints(0, download=False)
    return prob, opt


def timed(fn, repeats):
    fn()  # warm-up: buffers, page cache
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2), "repeats": repeats}


def kernel_stats(directory):
    """Per-save kernel time and device-to-host copy time from the rocpd database of a `--saves-only` run under rocprofv3."""
    dbs = sorted(glob.glob(os.path.join(directory, "**", "*results.db"), recursive=True))
    if not dbs:
        raise SystemExit(f"no *results.db under {directory}")
    cur = sqlite3.connect(dbs[0]).cursor()
    rows = cur.execute("select name, count(*), sum(end-start) from kernels group by name").fetchall()
    out = {"kernels_us": {}, "source": os.path.basename(dbs[0])}
    saves = 0
    for name, calls, total in rows:
        short = name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("dmsa::", "")
        if "k_pcd" in short or "scan" in short:
            out["kernels_us"][short] = {"calls": calls, "total_us": round(total / 1e3, 1)}
    try:
        copies = cur.execute("select count(*), sum(end-start), sum(size) from memory_copies where upper(name) like '%DEVICE_TO_HOST%' and size > 65536").fetchone()
        out["copy_back"] = {"copies": copies[0], "total_us": round((copies[1] or 0) / 1e3, 1), "bytes": copies[2]}
    except sqlite3.Error as e:  # the table is there only when the run had --memory-copy-trace
        out["copy_back"] = {"error": str(e)}
    return out, saves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", help="JSON file the figures are written to (merged into what it already holds)")
    ap.add_argument("--saves-only", type=int, default=0, help="only this many device saves to /dev/null: the run to put under rocprofv3")
    ap.add_argument("--kernel-stats", help="directory of a rocprofv3 --kernel-trace --memory-copy-trace --stats run of --saves-only")
    a = ap.parse_args()
    result = {}
    if a.out and os.path.exists(a.out):
        result = json.load(open(a.out))
    if a.kernel_stats:
        ks, _ = kernel_stats(a.kernel_stats)
        saves = result.get("profiled_saves") or 1
        ks["saves"] = saves
        ks["kernel_ms_per_save"] = round(sum(k["total_us"] for k in ks["kernels_us"].values()) / saves / 1e3, 3)
        if "total_us" in ks["copy_back"]:
            ks["copy_back_ms_per_save"] = round(ks["copy_back"]["total_us"] / saves / 1e3, 3)
            dev = result.get("device", {}).get("dev_null", {}).get("median_ms")
            if dev:
                ks["copy_back_share_of_dev_null_save"] = round(ks["copy_back_ms_per_save"] / dev, 3)
                ks["kernel_share_of_dev_null_save"] = round(ks["kernel_ms_per_save"] / dev, 3)
        result["profile"] = ks
    else:
        from dmsa_lidar_slam_amd import wire_formats as wf

        prob, opt = resident_map(a.frames)
        n = int(prob.localPoints.shape[0])
        if a.saves_only > 0:
            for _ in range(a.saves_only + 1):  # (+ the warm-up the timed runs have as well)
                wf.savePCDFileASCII("/dev/null", opt)
            result["profiled_saves"] = a.saves_only + 1
        else:
            with tempfile.TemporaryDirectory() as tmp:
                base = build_baseline(tmp)
                xyz, nrm = opt.globalPoints(), opt.getGlobalNormals()
                header = wf.pcdHeaderPointNormal(n).encode()
                fp = lambda arr: arr.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
                f_dev, f_base = os.path.join(tmp, "device.pcd"), os.path.join(tmp, "baseline.pcd")
                size = wf.savePCDFileASCII(f_dev, opt)
                assert base.baseline_save(f_base.encode(), header, fp(xyz), fp(nrm), n) == size
                same = open(f_dev, "rb").read() == open(f_base, "rb").read()
                result.update({
                    "map": {"frames": a.frames, "points": n, "file_bytes": size, "device_file_equals_baseline_file": bool(same)},
                    "device": {"dev_null": timed(lambda: wf.savePCDFileASCII("/dev/null", opt), a.repeats),
                               "local_file": timed(lambda: wf.savePCDFileASCII(f_dev, opt), a.repeats)},
                    "host_baseline_one_thread": {"dev_null": timed(lambda: base.baseline_save(b"/dev/null", header, fp(xyz), fp(nrm), n), a.repeats),
                                                 "local_file": timed(lambda: base.baseline_save(f_base.encode(), header, fp(xyz), fp(nrm), n), a.repeats)},
                })
                result["device_faster_than_baseline_to_dev_null"] = result["device"]["dev_null"]["median_ms"] < result["host_baseline_one_thread"]["dev_null"]["median_ms"]
        opt.close()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
