"""Time of the dense cloud (include/dmsa_dense_cloud.h) at the scan shape of the bench window: 131 072 points per message, 200 messages.

    python scripts/dense_cloud_time.py --out profiles/r09_dense_cloud.json        end to end (raw dump -> PCD on a local disk and -> /dev/null) vs the host baseline
    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format rocpd csv -d DIR -o dense -- examples/dense_cloud_from_raw DUMP POSES ouster /dev/null --voxel 0.1 --min-range 0.5
    python scripts/dense_cloud_time.py --kernel-stats DIR --out profiles/r09_dense_cloud.json     adds kernel-only time and the shares of that run
    python scripts/dense_cloud_time.py --intensity [--parent-example EXE] --out profiles/r19_dense_intensity.json
        the same workload with the intensity field of include/dmsa_dense_intensity.h: the example without the flag ("off"), with --intensity ("on") and,
        when given, the example of the parent commit, run in turn within every repeat, to /dev/null and to a local file; every run's figure is kept
    python scripts/dense_cloud_time.py --intensity --kernel-stats DIR_ON --kernel-stats-off DIR_OFF --out profiles/r19_dense_intensity.json
        adds from two profiler runs (the example with and without --intensity) what k_decode_field, the row packer and the copy-back cost

End to end is examples/dense_cloud_from_raw (no Python in the loop): the figure is the one it prints for its message loop -- read, upload,
kernels, copy-back, fwrite -- without the creation of the context.  `--keep DIR` leaves the dump and the poses there for the profiler run.
The baseline is ONE host thread doing the same arithmetic (the same include/dmsa_detmath.h, -ffp-contract=off, a std::unordered_set as the
voxel set) on the same decoded scans plus the same fwrite -- a small C++ helper this script builds.  No threshold is fixed in advance."""
import argparse
import ctypes as C
import glob
import json
import os
import re
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXAMPLE = os.path.join(ROOT, "examples", "dense_cloud_from_raw")

BASELINE_SRC = r"""
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <unordered_set>
#include <vector>
#include "dmsa_detmath.h"
// rules 1-7 of dmsa_dense_cloud.h on one thread; quat as (w, x, y, z), already normalised; identity lidar_to_imu
struct Baseline { std::unordered_set<uint64_t> seen; std::vector<float> rows; };
extern "C" void* baseline_new() { return new Baseline(); }
extern "C" void baseline_free(void* b) { delete static_cast<Baseline*>(b); }
extern "C" long long baseline_scan(void* bp, std::FILE* file, const float* xyz, const double* stamps, long long n, const double* s, const double* p, const double* q,
                                   int n_p, float min_range, float voxel) {
    Baseline& b = *static_cast<Baseline*>(bp);
    b.rows.clear();
    int j = 0;
    for (long long i = 0; i < n; ++i) {
        const float x = xyz[4 * i], y = xyz[4 * i + 1], z = xyz[4 * i + 2];
        const double t = stamps[i];
        if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(z) && std::isfinite(t))) continue;
        const float r = std::sqrt(x * x + (y * y + z * z));
        if (!(r > min_range) || !(t >= s[0] && t <= s[n_p - 1])) continue;
        while (j < n_p - 2 && s[j + 1] <= t) ++j;
        while (j > 0 && s[j] > t) --j;
        const double u = (t - s[j]) / (s[j + 1] - s[j]);
        const double *q1 = q + 4 * j, *q2 = q1 + 4;
        const double d = q1[0] * q2[0] + q1[1] * q2[1] + q1[2] * q2[2] + q1[3] * q2[3], ad = std::fabs(d);
        double s0, s1;
        if (ad >= 1.0 - DBL_EPSILON) s0 = 1.0 - u, s1 = u;
        else {
            const double th = dmsa_det::det_acos(ad), sn = dmsa_det::det_sin(th);
            s0 = dmsa_det::det_sin((1.0 - u) * th) / sn, s1 = dmsa_det::det_sin(u * th) / sn;
        }
        if (d < 0.0) s1 = -s1;
        const double qw = s0 * q1[0] + s1 * q2[0], qx = s0 * q1[1] + s1 * q2[1], qy = s0 * q1[2] + s1 * q2[2], qz = s0 * q1[3] + s1 * q2[3];
        double nn = std::sqrt(qx * qx + qy * qy + qz * qz), w[3] = {0, 0, 0};
        if (nn != 0.0) {
            const double angle = 2.0 * dmsa_det::det_atan2(nn, std::fabs(qw));
            if (qw < 0.0) nn = -nn;
            w[0] = qx / nn * angle, w[1] = qy / nn * angle, w[2] = qz / nn * angle;
        }
        double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        const double theta = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        if (!(theta < 0.00001)) {
            const double sn = dmsa_det::det_sin(theta) / theta, sh = dmsa_det::det_sin(0.5 * theta), c = 2.0 * sh * sh / (theta * theta), t2 = theta * theta;
            R[0] = 1.0 + c * (w[0] * w[0] - t2), R[4] = 1.0 + c * (w[1] * w[1] - t2), R[8] = 1.0 + c * (w[2] * w[2] - t2);
            R[1] = c * w[0] * w[1] - sn * w[2], R[3] = c * w[0] * w[1] + sn * w[2], R[2] = c * w[0] * w[2] + sn * w[1];
            R[6] = c * w[0] * w[2] - sn * w[1], R[5] = c * w[1] * w[2] - sn * w[0], R[7] = c * w[1] * w[2] + sn * w[0];
        }
        float g[3];
        for (int a = 0; a < 3; ++a) {
            const float tr = (float)(p[3 * j + a] + u * (p[3 * (j + 1) + a] - p[3 * j + a]));
            g[a] = (((float)R[3 * a] * x + (float)R[3 * a + 1] * y) + (float)R[3 * a + 2] * z) + tr;
        }
        if (voxel > 0.0f) {
            const float c0 = std::floor(g[0] / voxel), c1 = std::floor(g[1] / voxel), c2 = std::floor(g[2] / voxel), lim = 1048576.0f;
            if (!(c0 >= -lim && c0 < lim && c1 >= -lim && c1 < lim && c2 >= -lim && c2 < lim)) continue;
            const uint64_t key = ((uint64_t)((int)c0 + 1048576) << 42) | ((uint64_t)((int)c1 + 1048576) << 21) | (uint64_t)((int)c2 + 1048576);
            if (!b.seen.insert(key).second) continue;
        }
        b.rows.insert(b.rows.end(), g, g + 3);
    }
    if (file && std::fwrite(b.rows.data(), 4, b.rows.size(), file) != b.rows.size()) return -1;
    return (long long)(b.rows.size() / 3);
}
extern "C" std::FILE* baseline_open(const char* path) { return std::fopen(path, "wb"); }
extern "C" int baseline_close(std::FILE* f) { return std::fclose(f); }
"""

OUSTER = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad0", "<f4"), ("intensity", "<f4"), ("t", "<u4"), ("reflectivity", "<u2"), ("ring", "u1"),
                   ("pad1", "u1"), ("ambient", "<u2"), ("pad2", "<u2"), ("range", "<u4")])
OUSTER_FIELDS = ["x", "y", "z", "intensity", "t", "reflectivity", "ring", "ambient", "range"]


def make_sequence(directory, messages, points, seed=1, intensity=False):
    """A drive along a smooth path: `messages` Ouster messages of `points` points at 10 Hz (a 128-ring sweep of a 40 m room, stamps rising through
    the sweep), the raw dump, and a Poses.txt with one pose per message boundary."""
    from dmsa_lidar_slam_amd import raw_sequence as rs
    from dmsa_lidar_slam_amd import wire_formats as wf

    rng = np.random.default_rng(seed)
    dump, poses = os.path.join(directory, "sequence.raw"), os.path.join(directory, "Poses.txt")
    t0 = 1.6e9
    with open(poses, "w") as f:
        for k in range(messages + 1):
            s = 0.1 * k
            f.write(wf.addPoseToFile(t0 + s, [1.5 * s, 2.0 * np.sin(0.2 * s), 0.1 * np.cos(0.3 * s)], [0.02 * np.sin(s), 0.03 * np.cos(0.7 * s), 0.25 * s]))
    rings = 128
    az = points // rings
    el = np.repeat(np.linspace(-0.39, 0.39, rings), az)
    phi = np.tile(np.linspace(0, 2 * np.pi, az, endpoint=False), rings)
    direction = np.stack([np.cos(el) * np.cos(phi), np.cos(el) * np.sin(phi), np.sin(el)], axis=1)
    offs = np.array([OUSTER.fields[n][1] for n in OUSTER_FIELDS], np.uint32)
    scans = []
    with rs.RawWriter(dump) as w:
        for k in range(messages):
            rec = np.zeros(direction.shape[0], OUSTER)
            rng_m = np.minimum(20.0 / np.maximum(np.abs(direction[:, 0]), np.abs(direction[:, 1])), 3.0 / np.maximum(np.abs(direction[:, 2]), 1e-3))
            xyz = (direction * (rng_m + rng.normal(0, 0.01, rng_m.shape))[:, None]).astype(np.float32)
            rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
            rec["t"] = np.tile(np.linspace(0, 0.1e9, az, endpoint=False), rings).astype(np.uint32)
            rec["ring"] = np.repeat(np.arange(rings), az)
            if intensity:  # something to carry: brighter close by
                rec["intensity"] = (255.0 / (1.0 + 0.1 * rng_m)).astype(np.float32)
            msg = wf.PointCloud2Msg(height=1, width=rec.shape[0], point_step=OUSTER.itemsize, field_offsets=offs, data=np.frombuffer(rec.tobytes(), np.uint8),
                                    stamp=t0 + 0.1 * k)
            w.writePointCloud2(msg)
            if k < 8:  # the baseline walks these decoded scans again and again
                scans.append((np.concatenate([xyz, np.zeros((xyz.shape[0], 1), np.float32)], axis=1), t0 + 0.1 * k + 1e-9 * rec["t"].astype(np.float64)))
    return dump, poses, scans


def run_example(dump, poses, out, voxel, min_range, exe=EXAMPLE, flags=()):
    p = subprocess.run([exe, dump, poses, "ouster", out, "--voxel", str(voxel), "--min-range", str(min_range), *flags], capture_output=True, text=True, check=True)
    m = re.search(r"(\d+) points, (\d+) bytes; ([0-9.]+) s", p.stdout)
    points_in = int(re.search(r"points_in (\d+)", p.stdout).group(1))
    return {"points_in": points_in, "points_out": int(m.group(1)), "bytes": int(m.group(2)), "seconds": float(m.group(3))}


def median_of(fn, repeats):
    fn()  # warm-up: page cache, first-touch of the buffers
    runs = [fn() for _ in range(repeats)]
    sec = statistics.median(r["seconds"] for r in runs)
    return {**runs[0], "seconds": None, "median_s": round(sec, 4), "min_s": round(min(r["seconds"] for r in runs), 4), "max_s": round(max(r["seconds"] for r in runs), 4),
            "repeats": repeats, "points_in_per_s": round(runs[0]["points_in"] / sec)}


def spread_of(runs):
    sec = [r["seconds"] for r in runs]
    return {**runs[0], "seconds": None, "runs_s": [round(s, 4) for s in sec], "median_s": round(statistics.median(sec), 4), "min_s": round(min(sec), 4),
            "max_s": round(max(sec), 4), "points_in_per_s": round(runs[0]["points_in"] / statistics.median(sec))}


def intensity_runs(a, dump, poses, tmp):
    """off / on / parent in turn within every repeat (one warm-up round first), so that a drift of the machine meets all three alike."""
    variants = {"off": (EXAMPLE, ()), "on": (EXAMPLE, ("--intensity",))}
    if a.parent_example:
        variants["parent"] = (a.parent_example, ())
    runs = {v: {"dev_null": [], "local_file": []} for v in variants}
    for rep in range(a.repeats + 1):
        for v, (exe, flags) in variants.items():
            for target, out in (("dev_null", "/dev/null"), ("local_file", os.path.join(tmp, v + ".pcd"))):
                r = run_example(dump, poses, out, a.voxel, a.min_range, exe, flags)
                if rep > 0:
                    runs[v][target].append(r)
    out = {v: {t: spread_of(rs) for t, rs in targets.items()} for v, targets in runs.items()}
    if a.parent_example:  # the off path launches the parent's kernels: the two ranges have to overlap
        out["off_range_overlaps_parent"] = {t: out["off"][t]["min_s"] <= out["parent"][t]["max_s"] and out["parent"][t]["min_s"] <= out["off"][t]["max_s"]
                                            for t in ("dev_null", "local_file")}
        out["off_file_equals_parent_file"] = open(os.path.join(tmp, "off.pcd"), "rb").read() == open(os.path.join(tmp, "parent.pcd"), "rb").read()
    d = {t: out["on"][t]["median_s"] - out["off"][t]["median_s"] for t in ("dev_null", "local_file")}
    out["on_minus_off_s"] = {"dev_null": round(d["dev_null"], 4), "local_file": round(d["local_file"], 4),
                             "write_share_s": round(d["local_file"] - d["dev_null"], 4)}  # what the larger rows cost on the way to the disk
    return out


def intensity_profile(dir_on, dir_off):
    """From two profiler runs of the example: what the on path adds in kernels and in the copy-back."""
    on, off = kernel_stats(dir_on), kernel_stats(dir_off)
    us = lambda ks, name: sum(v["total_us"] for k, v in ks["kernels_us"].items() if k.startswith(name))  # noqa: E731
    return {"on": on, "off": off,
            "added_s": {"k_decode_field": round(us(on, "k_decode_field") / 1e6, 5),
                        "k_dense_pack_rows": round((us(on, "k_dense_pack_rows") - us(off, "k_dense_pack_rows")) / 1e6, 5),
                        "k_dense_place": round((us(on, "k_dense_place") - us(off, "k_dense_place")) / 1e6, 5),
                        "all_kernels": round(on["kernel_s"] - off["kernel_s"], 5),
                        "copy_back": round(on.get("copy_back", {}).get("total_s", 0.0) - off.get("copy_back", {}).get("total_s", 0.0), 5)}}


def build_baseline(tmp):
    src, lib = os.path.join(tmp, "dense_baseline.cpp"), os.path.join(tmp, "libdense_baseline.so")
    with open(src, "w") as f:
        f.write(BASELINE_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-o", lib, src])
    L = C.CDLL(lib)
    L.baseline_new.restype = L.baseline_open.restype = C.c_void_p
    L.baseline_free.argtypes = [C.c_void_p]
    L.baseline_open.argtypes = [C.c_char_p]
    L.baseline_close.argtypes = [C.c_void_p]
    L.baseline_scan.restype = C.c_longlong
    L.baseline_scan.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                C.POINTER(C.c_double), C.c_int, C.c_float, C.c_float]
    return L


def run_baseline(L, scans, poses, out, voxel, min_range, messages):
    """The first `messages` scans on one host thread (the decoded scans are handed over: the byte decoding is not in the baseline's time)."""
    from dmsa_lidar_slam_amd.dense_cloud import parse_tum_poses

    s, p, q = parse_tum_poses(open(poses, "rb").read())
    q = q / np.sqrt((q * q).sum(axis=1))[:, None]
    q = np.ascontiguousarray(np.concatenate([q[:, 3:], q[:, :3]], axis=1))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    b, f = L.baseline_new(), L.baseline_open(out.encode())
    kept, t0 = 0, time.perf_counter()
    for k in range(messages):
        xyz, st = scans[k % len(scans)]
        st = st + 0.1 * (k - k % len(scans))
        kept += L.baseline_scan(b, f, xyz.ctypes.data_as(C.POINTER(C.c_float)), dp(st), xyz.shape[0], dp(s), dp(p), dp(q), s.shape[0], min_range, voxel)
    L.baseline_close(f)
    sec = time.perf_counter() - t0
    L.baseline_free(b)
    return {"points_in": messages * scans[0][0].shape[0], "points_out": int(kept), "seconds": sec}


def _short(name):
    return name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("dmsa::", "")


def kernel_stats(directory):
    """Kernel and copy time per category of a run of the example under rocprofv3: from its rocpd database, or from the *_stats.csv files."""
    out = {"kernels_us": {}}
    dbs = sorted(glob.glob(os.path.join(directory, "**", "*results.db"), recursive=True))
    try:
        cur = sqlite3.connect(dbs[0]).cursor()
        for name, calls, total in cur.execute("select name, count(*), sum(end-start) from kernels group by name").fetchall():
            out["kernels_us"][_short(name)] = {"calls": calls, "total_us": round(total / 1e3, 1)}
        for tag, like in (("upload", "%HOST_TO_DEVICE%"), ("copy_back", "%DEVICE_TO_HOST%")):
            n, total, size = cur.execute("select count(*), sum(end-start), sum(size) from memory_copies where upper(name) like ?", (like,)).fetchone()
            out[tag] = {"copies": n, "total_s": round((total or 0) / 1e9, 4), "bytes": size}
        out["source"] = os.path.basename(dbs[0])
    except (IndexError, sqlite3.Error):
        import csv

        out = {"kernels_us": {}, "source": "csv"}
        for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                out["kernels_us"][_short(row["Name"])] = {"calls": int(row["Calls"]), "total_us": round(float(row["TotalDurationNs"]) / 1e3, 1)}
        for path in glob.glob(os.path.join(directory, "**", "*memory_copy_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                tag = "upload" if "HOST_TO_DEVICE" in row["Name"].upper() else "copy_back" if "DEVICE_TO_HOST" in row["Name"].upper() else None
                if tag:
                    out[tag] = {"copies": int(row["Calls"]), "total_s": round(float(row["TotalDurationNs"]) / 1e9, 4)}
        if not out["kernels_us"]:
            raise SystemExit(f"neither a readable *results.db nor *kernel_stats.csv under {directory}")
    out["kernel_s"] = round(sum(k["total_us"] for k in out["kernels_us"].values()) / 1e6, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--min-range", type=float, default=0.5)
    ap.add_argument("--baseline-messages", type=int, default=20, help="messages the one-thread baseline walks (its rate is per point)")
    ap.add_argument("--keep", help="write the dump and the poses here and leave them (for the profiler run)")
    ap.add_argument("--out", help="JSON file the figures are written to (merged into what it already holds)")
    ap.add_argument("--kernel-stats", help="directory of a rocprofv3 --kernel-trace --memory-copy-trace --stats run of the example")
    ap.add_argument("--intensity", action="store_true", help="time the example with and without --intensity (and the parent's example) instead of the host baseline")
    ap.add_argument("--parent-example", help="with --intensity: the dense_cloud_from_raw of the parent commit, run in turn with this one's")
    ap.add_argument("--kernel-stats-off", help="with --intensity --kernel-stats: the profiler run of the example without --intensity")
    a = ap.parse_args()
    result = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    if a.intensity and a.kernel_stats:
        result["profile"] = intensity_profile(a.kernel_stats, a.kernel_stats_off)
    elif a.intensity:
        with tempfile.TemporaryDirectory() as tmp:
            work = a.keep or tmp
            os.makedirs(work, exist_ok=True)
            dump, poses, _ = make_sequence(work, a.messages, a.points, intensity=True)
            result.update({"workload": {"messages": a.messages, "points_per_message": a.points, "voxel_size": a.voxel, "min_range": a.min_range,
                                        "dump_bytes": os.path.getsize(dump), "repeats": a.repeats, "order": "off, on, parent within every repeat; one warm-up round"},
                           "device": intensity_runs(a, dump, poses, tmp)})
    elif a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        e2e = result.get("device", {}).get("dev_null", {})
        if e2e.get("median_s"):
            ks["share_of_dev_null_run"] = {k: round(v / e2e["median_s"], 3) for k, v in (("kernels", ks["kernel_s"]), ("upload", ks.get("upload", {}).get("total_s", 0.0)),
                                                                                         ("copy_back", ks.get("copy_back", {}).get("total_s", 0.0)))}
            ks["kernel_only_points_in_per_s"] = round(e2e["points_in"] / ks["kernel_s"]) if ks["kernel_s"] else None
        result["profile"] = ks
    else:
        with tempfile.TemporaryDirectory() as tmp:
            work = a.keep or tmp
            os.makedirs(work, exist_ok=True)
            dump, poses, scans = make_sequence(work, a.messages, a.points)
            f_dev, f_base = os.path.join(tmp, "device.pcd"), os.path.join(tmp, "baseline.pcd")
            L = build_baseline(tmp)
            result.update({
                "workload": {"messages": a.messages, "points_per_message": a.points, "voxel_size": a.voxel, "min_range": a.min_range, "dump_bytes": os.path.getsize(dump)},
                "device": {"dev_null": median_of(lambda: run_example(dump, poses, "/dev/null", a.voxel, a.min_range), a.repeats),
                           "local_file": median_of(lambda: run_example(dump, poses, f_dev, a.voxel, a.min_range), a.repeats)},
                "host_baseline_one_thread": {"messages": a.baseline_messages,
                                             "dev_null": median_of(lambda: run_baseline(L, scans, poses, "/dev/null", a.voxel, a.min_range, a.baseline_messages), a.repeats),
                                             "local_file": median_of(lambda: run_baseline(L, scans, poses, f_base, a.voxel, a.min_range, a.baseline_messages), a.repeats)},
            })
            result["device_faster_than_baseline_to_dev_null"] = (result["device"]["dev_null"]["points_in_per_s"] >
                                                                 result["host_baseline_one_thread"]["dev_null"]["points_in_per_s"])
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
