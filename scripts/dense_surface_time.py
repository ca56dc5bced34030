"""Time of the dense cloud's fused surface (include/dmsa_dense_surface.h) on the workload of profiles/r09_dense_cloud.json: 200 Ouster messages of
131 072 points, voxel 0.1 m; the default config (cells of 0.2 m, truncation 0.6 m, max_length 30 m, min_weight 2).

    python scripts/dense_surface_time.py --out profiles/r30_dense_surface.json
    rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- python scripts/dense_surface_time.py --kernels-only
    python scripts/dense_surface_time.py --trace DIR --out profiles/r30_dense_surface.json --stats-out profiles/r30_dense_surface_kernel_stats.txt

End to end is dmsa_dense_cloud_build_surface on a store whose search grid has the cells' edge already (build_occupancy with the same cell ran
before it): the table cleared, k_surface_integrate, the small read, the listing (flags, scan, compaction, 64-bit sort, sums and weights in
order) and the final read; median of 5 after a warm-up.  The statistics must be the same integers in every run.  Beside it, in the same process
on the same store: build_occupancy, extract_mesh, and the two writers to /dev/null.
The kernel figures come from ONE rocprofv3 --kernel-trace run of --kernels-only (no counters are collected in it): k_surface_integrate against
k_occupancy_walk of the same process, which walks every ray whole where the surface walks two truncations of it.  No ratio is fixed in
advance."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_cloud_time as dct  # noqa: E402  (the sequence generator)
from dense_normals_time import spread, timed  # noqa: E402

KERNELS = ("k_surface_integrate", "k_occupancy_walk", "k_surface_clear", "k_surface_flags", "k_surface_compact", "k_surface_list", "k_surface_rows", "k_mesh_mark",
           "k_mesh_count", "k_mesh_emit", "k_mesh_face_rows")


def trace_rows(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(open(path))]
    rows.sort()
    return rows


def trace_figures(rows):
    """Durations [ms] per kernel of a rocprofv3 --kernel-trace run; the first dispatch of each (the warm-up) left out."""
    out = {}
    for name in KERNELS:
        ms = [d / 1e3 for _, kernel, d in rows if name + "(" in kernel][1:]
        if ms:
            out[name + "_ms"] = {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "dispatches": len(ms)}
    if "k_surface_integrate_ms" in out and "k_occupancy_walk_ms" in out:
        out["integrate_over_occupancy_walk"] = round(out["k_surface_integrate_ms"]["median"] / out["k_occupancy_walk_ms"]["median"], 2)
    return out


def stats_text(rows, head):
    """The table of a kernel-stats file: every dispatch of the stage's kernels, durations in us."""
    lines = [head, "", f"{'kernel':<40}{'calls':>8}{'total_us':>12}{'avg_us':>11}{'min_us':>11}{'max_us':>11}"]
    table = []
    for name in KERNELS:
        us = [d for _, kernel, d in rows if name + "(" in kernel]
        if us:
            table.append((sum(us), f"{'dmsa::' + name:<40}{len(us):>8}{sum(us):>12.1f}{sum(us) / len(us):>11.2f}{min(us):>11.2f}{max(us):>11.2f}"))
    return "\n".join(lines + [line for _, line in sorted(table, reverse=True)]) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--min-range", type=float, default=0.5)
    ap.add_argument("--kernels-only", action="store_true", help="the device work alone, for a profiler run (the same calls: nothing else is timed here)")
    ap.add_argument("--trace", help="the output directory of a rocprofv3 --kernel-trace run of --kernels-only: its per-kernel figures are merged into --out")
    ap.add_argument("--stats-out", help="with --trace: the text file the per-kernel table is written to")
    ap.add_argument("--out", help="JSON file the figures are written to (merged into what it already holds)")
    a = ap.parse_args()
    result = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    if a.trace:
        rows = trace_rows(a.trace)
        result["kernels_from_one_kernel_trace_run"] = trace_figures(rows)
        if a.stats_out:
            rows_n = result.get("workload", {}).get("retained_rows", "?")
            head = ("Per-kernel times of the dense cloud's fused surface beside the occupancy walk (include/dmsa_dense_surface.h, include/dmsa_dense_occupancy.h), from one\n"
                    "rocprofv3 --kernel-trace --stats run on an MI355X (no counters) of scripts/dense_surface_time.py --kernels-only: the workload of\n"
                    f"{os.path.basename(a.out or 'the JSON beside this file')} ({rows_n} retained rows, cells of 0.2 m), a warm-up and {a.repeats} timed calls each of build_occupancy,\n"
                    "build_surface, extract_mesh and the two writers to /dev/null, in one process.  Durations in us.  The scan and sort kernels are the library's own\n"
                    "and serve the store's fill and the search grid as well; they, the kernels that fill the store and the runtime's copies and fills are left out.")
            with open(a.stats_out, "w") as f:
                f.write(stats_text(rows, head))
    else:
        from dmsa_lidar_slam_amd import raw_sequence as rs
        from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator, DenseOccupancyConfig, DenseSurfaceConfig

        cfg, occupancy = DenseSurfaceConfig(), DenseOccupancyConfig()
        with tempfile.TemporaryDirectory() as tmp:
            dump, poses, _ = dct.make_sequence(tmp, a.messages, a.points)
            dc = DenseCloudCreator.from_tum_file(poses, DenseCloudConfig(minRange=a.min_range, voxelSize=a.voxel), retain=True)
            for kind, msg in rs.RawReader(dump):
                if kind == "pointcloud2":
                    dc.add_pointcloud2(msg, "ouster", download=False)
            n = dc.retained_count()
            print(f"store: {n} rows", flush=True)
            dc.build_occupancy(occupancy)  # warm-up, and the grid at the cells' edge
            t_occupancy = spread([timed(lambda: dc.build_occupancy(occupancy))[0] for _ in range(a.repeats)])
            _, stats = timed(lambda: dc.build_surface(cfg))  # warm-up: code objects, buffers
            runs = [timed(lambda: dc.build_surface(cfg)) for _ in range(a.repeats)]
            assert all(r[1] == stats for r in runs)  # the same integers every run
            _, mesh = timed(lambda: dc.extract_mesh(cfg.min_weight))
            meshes = [timed(lambda: dc.extract_mesh(cfg.min_weight)) for _ in range(a.repeats)]
            assert all(r[1] == mesh for r in meshes)
            dc.save_pcd_tsdf("/dev/null")
            voxels = [timed(lambda: dc.save_pcd_tsdf("/dev/null")) for _ in range(a.repeats)]
            dc.save_ply_mesh("/dev/null")
            plys = [timed(lambda: dc.save_ply_mesh("/dev/null")) for _ in range(a.repeats)]
            figures = {"build_surface": spread([r[0] for r in runs]), "build_occupancy_same_process": t_occupancy, "extract_mesh": spread([r[0] for r in meshes]),
                       "save_pcd_tsdf": spread([r[0] for r in voxels]), "save_ply_mesh": spread([r[0] for r in plys]), "voxel_file_bytes": 20 * stats["cells"],
                       "mesh_file_bytes": 12 * mesh["vertices"] + 13 * mesh["triangles"], "rays_per_s": round(n / statistics.median([r[0] for r in runs]))}
            print("device:", json.dumps(figures), json.dumps(stats), json.dumps(mesh), flush=True)
            result.update({"workload": {"messages": a.messages, "points_per_message": a.points, "voxel_size": a.voxel, "min_range": a.min_range, "retained_rows": n,
                                        "config": {k: getattr(cfg, k) for k in ("cell_size", "truncation", "max_length", "min_weight")}},
                           "counts": stats, "mesh": mesh, "device": figures, "not_measured": "hardware counters; the wave merge of equal cells before the atomics"})
            dc.close()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
