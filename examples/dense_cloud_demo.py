"""The step after the run, on the synthetic drive of sequence_demo.py: the run records its message stream and writes its TUM lines; the dense
cloud then walks the recording again, places EVERY raw point at the pose interpolated for its own stamp, thins to one point per voxel and
writes a binary PCD (include/dmsa_dense_cloud.h).  Run:  python examples/dense_cloud_demo.py [--scans 10] [--out DenseCloud.pcd]
With --outliers K MUL the retained survivors go through statistical outlier removal first (include/dmsa_dense_outliers.h) and the cleaned store
is written as a second x y z file; with --normals RADIUS as well, the normals are those of the cleaned store.
With --carve [CELL RHO PASSES] moving objects are removed first of all (include/dmsa_dense_carve.h): every retained point that at least PASSES
rays of other points pass straight through leaves the store, so that neither the outlier statistic nor the normals see it.  The stages compose
in the order carve, --clusters, --outliers, --compare, --normals.
With --clusters RADIUS MIN_SIZE the store is split into its Euclidean clusters (include/dmsa_dense_clusters.h: connected components of "at most
RADIUS apart"), the clusters of fewer than MIN_SIZE points leave it -- what carving left of a moving object is such a blob -- and the cleaned
store is written with a `label` field, the cluster of every point.
With --compare PATH the store is compared with a reference cloud (include/dmsa_dense_compare.h; any binary PCD with x y z fields, such as a file
of an earlier run): nearest distances in both directions up to --compare-max, precision, recall and F-score at --compare-tol (both defaults are
placeholders from no recorded data), and the store written with a `distance` field.
With --align as well the reference is first aligned to the store by ICP (include/dmsa_dense_align.h; with --align-metric plane by point to
plane, include/dmsa_dense_align_plane.h, on the store's normals, which are computed first) with --compare-max as the reach of the
pairs.  To have something to align, --compare-displace DEG,M moves the reference file's rows by a known rigid motion (DEG degrees about a fixed
oblique axis through the cloud's centre, then M metres along another) before they are used; the demo prints the motion it recovered beside the
inverse of the one it applied.
With --occupancy [CELL] the rays of the rows still in the store, after --carve, --clusters and --outliers and before --normals, are walked into an
occupancy map (include/dmsa_dense_occupancy.h): every cell seen occupied, seen free or left unknown, written as DenseCloudOccupancy.pcd (x y z hits
passes state); with --occupancy-slice LO HI as well, the cells between the two heights are projected into map.pgm + map.yaml, the pair the ROS
map_server loads.  Thinning and every removal take their rays with them: only what is left in the store is evidence.
With --mesh [CELL] the same rays, at the same place in the order, are fused into a truncated signed distance field with cells of CELL metres and a
truncation of three cells (include/dmsa_dense_surface.h), and its zero set is written as DenseCloudMesh.ply (binary PLY, triangles); --tsdf-out
also writes the field itself as x y z tsdf weight.
With --intensity every file gets an `intensity` field after z (include/dmsa_dense_intensity.h): the synthetic scene has no reflectance of its own,
so the demo paints one per surface orientation into the messages' intensity field before it replays them -- something to look at, no more.
"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import sequence_demo  # noqa: E402

from dmsa_lidar_slam_amd import raw_sequence as rs, synth  # noqa: E402
from dmsa_lidar_slam_amd.dense_cloud import DenseCarveConfig, DenseCloudConfig, DenseCloudCreator, DenseOccupancyConfig, DenseSurfaceConfig, read_pcd_xyz  # noqa: E402


def displacement(deg, metres, centre):
    """The 3x4 rigid motion of --compare-displace: deg degrees about the axis (0.2, -0.3, 1) through `centre`, then metres along (0.6, -0.48, 0.64)."""
    axis = np.array([0.2, -0.3, 1.0]) / np.linalg.norm([0.2, -0.3, 1.0])
    a = np.radians(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    t = np.asarray(centre, np.float64) - R @ np.asarray(centre, np.float64) + metres * np.array([0.6, -0.48, 0.64])
    return np.concatenate([R, t.reshape(3, 1)], axis=1)


def inverse_motion(T):
    return np.concatenate([T[:, :3].T, -(T[:, :3].T @ T[:, 3:])], axis=1)


REFLECTANCE = np.array([12.0, 18.0, 35.0, 42.0, 80.0, 65.0], np.float32)  # by the surface's outward normal: -x +x -y +y -z (ceilings) +z (floors, treads)


def surface_reflectance(scans, seed=1, rings=64, az_steps=512):
    """One float32 array per scan of the synthetic drive: a fixed reflectance per surface orientation, found by casting every ray of the scan
    again from the true pose.  Deterministic; there is no accuracy claim on it."""
    clouds, truth = synth.scan_sequence(seed=seed, scans=scans, rings=rings, az_steps=az_steps)
    scene = synth.Scene.room_with_stairs()
    out = []
    for xyz, stamps, _, _ in clouds:
        R, p = truth.pose(stamps - 1.6e9)
        d = R.apply(xyz.astype(np.float64))
        _, nrm = scene.raycast(p, d / np.linalg.norm(d, axis=1, keepdims=True))
        axis = np.argmax(np.abs(nrm), axis=1)
        out.append(REFLECTANCE[2 * axis + (nrm[np.arange(axis.shape[0]), axis] > 0)])
    return out


def paint(msg, values):
    """The Ouster message with `values` in its intensity field (field 3, float32)."""
    if values.shape[0] != int(msg.height) * int(msg.width):
        raise ValueError("the recording does not hold the synthetic drive's scans")
    rec = np.frombuffer(np.ascontiguousarray(msg.data, np.uint8).tobytes(), sequence_demo.OUSTER).copy()
    rec["intensity"] = values
    msg.data = np.frombuffer(rec.tobytes(), np.uint8).copy()
    return msg


def run(scans=10, out=None, workdir=None, voxel_size=0.1, min_range=0.5, normals=None, normals_out=None, outliers=None, outlier_radius=None, clean_out=None, carve=None, carved_out=None,
        intensity=False, clusters=None, clusters_out=None, compare=None, compare_max=1.0, compare_tol=0.1, compare_out=None, align=False, align_metric="point",
        compare_displace=None, occupancy=None, occupancy_out=None, occupancy_slice=None, map_out=None, occupancy_rays_out=None, mesh=None, mesh_out=None, tsdf_out=None, **run_args):
    """Returns the statistics of the dense cloud, the points and bytes of the file, and the paths.  normals = a radius [m]: the survivors are
    retained and a second, seven-field file with a normal and a curvature per point is written (include/dmsa_dense_normals.h).
    outliers = (k, stddev_mul): the retained survivors are classified (search radius outlier_radius, default the normals' radius or three
    voxels), the outliers removed from the store and the cleaned store written as x y z (include/dmsa_dense_outliers.h); normals then are
    those of the cleaned store.  carve = a DenseCarveConfig (or True for the defaults): before either, the rows that min_passes rays see through
    are removed from the store and the store written as x y z (include/dmsa_dense_carve.h).  clusters = (radius, min_size): after the carving
    and before the outliers, the clusters of fewer than min_size rows are removed and the store is written as x y z label
    (include/dmsa_dense_clusters.h).  compare = the path of a reference cloud (a binary PCD with x y z fields): after the outliers and before
    the normals the store is compared with it, nearest distances both ways up to compare_max with precision, recall and f_score at compare_tol,
    and written as x y z distance (include/dmsa_dense_compare.h).  compare_displace = (degrees, metres): the reference rows are moved by
    displacement() first; align: the reference is aligned to the store by ICP before the comparison (include/dmsa_dense_align.h; align_metric="plane": point to plane,
    include/dmsa_dense_align_plane.h, on the normals of the store at the radius `normals` or 0.3 m, computed first).  intensity: every file has an `intensity` field
    after z (include/dmsa_dense_intensity.h), read from the messages' own field.  occupancy = a DenseOccupancyConfig (or True for the defaults): after
    the outliers and before the comparison the occupancy map of the store's rays is built and written as x y z hits passes state
    (include/dmsa_dense_occupancy.h); occupancy_slice = (z_lo, z_hi): its cells between the two heights go to map_out (a .pgm) and the .yaml beside it;
    occupancy_rays_out: the rays the map was built from, the store's points and origins, as an .npz (xyz, origin).  mesh = a DenseSurfaceConfig (or
    True for the defaults): at the same place the signed distance field of the store's rays is built and its zero set written to mesh_out as a PLY
    (include/dmsa_dense_surface.h); tsdf_out: the field as x y z tsdf weight."""
    workdir = workdir or tempfile.mkdtemp(prefix="dense_cloud_demo_")
    dump, poses = os.path.join(workdir, "sequence.raw"), os.path.join(workdir, "Poses.txt")
    out = out or os.path.join(workdir, "DenseCloud.pcd")
    r = sequence_demo.run(scans=scans, record=dump, **run_args)  # Ouster messages
    with open(poses, "w") as f:
        f.write("".join(r["tum"]))
    dc = DenseCloudCreator.from_tum_file(poses, DenseCloudConfig(minRange=min_range, voxelSize=voxel_size), retain=normals is not None or outliers is not None or carve is not None or clusters is not None or compare is not None or occupancy is not None or mesh is not None,
                                       intensity=intensity)
    painted = surface_reflectance(scans, **{k: run_args[k] for k in ("seed", "rings", "az_steps") if k in run_args}) if intensity else None
    extra = {}
    try:
        dc.open_pcd(out)
        n_scans = 0
        for kind, msg in rs.RawReader(dump):
            if kind == "pointcloud2":
                if intensity:
                    dc.add_pointcloud2(paint(msg, painted[n_scans]), "ouster", download=False, intensity_field="auto")
                else:
                    dc.add_pointcloud2(msg, "ouster", download=False)
                n_scans += 1
        points, size = dc.close_pcd()
        stats = dc.stats()
        if carve is not None:
            carved_out = carved_out or os.path.join(workdir, "DenseCloudCarved.pcd")
            cfg = DenseCarveConfig() if carve is True else carve
            t_stats = dc.count_passes(cfg)
            left = dc.remove_transients()
            t_points, t_bytes = dc.save_pcd_retained(carved_out)
            assert left == t_points == t_stats["kept"]
            extra = {"carve": t_stats, "carve_config": cfg, "carved_pcd": carved_out, "carved_points": t_points, "carved_bytes": t_bytes}
        if clusters is not None:
            clusters_out = clusters_out or os.path.join(workdir, "DenseCloudClusters.pcd")
            c_radius, c_min = float(clusters[0]), int(clusters[1])
            k_stats = dc.classify_clusters(radius=c_radius, min_size=c_min)
            left = dc.remove_clusters()
            dc.cluster_labels(c_radius)  # of the cleaned store: the labels of the file
            k_points, k_bytes = dc.save_pcd_labels(clusters_out)
            assert left == k_points == k_stats["kept_rows"]
            extra.update({"clusters": k_stats, "clusters_pcd": clusters_out, "clusters_points": k_points, "clusters_bytes": k_bytes})
        if outliers is not None:
            clean_out = clean_out or os.path.join(workdir, "DenseCloudClean.pcd")
            radius = outlier_radius or normals or 3.0 * voxel_size
            o_stats = dc.classify_outliers(radius=radius, k=int(outliers[0]), stddev_mul=float(outliers[1]))
            left = dc.remove_outliers()
            c_points, c_bytes = dc.save_pcd_retained(clean_out)
            assert left == c_points == o_stats["inliers"]
            extra.update({"outliers": o_stats, "outlier_radius": radius, "clean_pcd": clean_out, "clean_points": c_points, "clean_bytes": c_bytes})
        if occupancy is not None:
            occupancy_out = occupancy_out or os.path.join(workdir, "DenseCloudOccupancy.pcd")
            cfg = DenseOccupancyConfig() if occupancy is True else occupancy
            m_stats = dc.build_occupancy(cfg)
            m_rows = dc.save_pcd_occupancy(occupancy_out, 0)
            assert m_rows == m_stats["cells"]
            extra.update({"occupancy": m_stats, "occupancy_config": cfg, "occupancy_pcd": occupancy_out})
            if occupancy_rays_out:
                g, o = dc.retained()
                np.savez(occupancy_rays_out, xyz=g, origin=o)
            if occupancy_slice is not None:
                map_out = map_out or os.path.join(workdir, "map.pgm")
                yaml_out = os.path.splitext(map_out)[0] + ".yaml"
                info, _ = dc.occupancy_slice(*occupancy_slice)
                dc.save_occupancy_map(map_out, yaml_out, *occupancy_slice)
                extra.update({"map": info, "map_pgm": map_out, "map_yaml": yaml_out})
        if mesh is not None:
            mesh_out = mesh_out or os.path.join(workdir, "DenseCloudMesh.ply")
            cfg = DenseSurfaceConfig() if mesh is True else mesh
            s_stats = dc.build_surface(cfg)
            f_stats = dc.extract_mesh(cfg.min_weight)
            dc.save_ply_mesh(mesh_out)
            extra.update({"surface": s_stats, "surface_config": cfg, "mesh": f_stats, "mesh_ply": mesh_out})
            if tsdf_out:
                assert dc.save_pcd_tsdf(tsdf_out) == s_stats["cells"]
                extra.update({"tsdf_pcd": tsdf_out})
        if compare is not None:
            compare_out = compare_out or os.path.join(workdir, "DenseCloudDistance.pcd")
            ref = read_pcd_xyz(compare)
            if compare_displace is not None:
                applied = displacement(float(compare_displace[0]), float(compare_displace[1]), ref.mean(axis=0))
                ref = (ref.astype(np.float64) @ applied[:, :3].T + applied[:, 3]).astype(np.float32)
                extra.update({"applied": applied})
            if align and align_metric == "plane":  # P0: the normals of the store as it stands, at --normals' radius or 0.3 m
                dc.compute_normals(radius=normals if normals is not None else 0.3, download=False)
            if align:
                extra.update({"align": dc.align_reference(ref, max_distance=compare_max, metric=align_metric)})
            else:
                dc.set_reference(ref)
            m_stats = dc.compare(max_distance=compare_max, tolerance=compare_tol)
            m_points, m_bytes = dc.save_pcd_distance(compare_out)
            extra.update({"compare": m_stats, "distance_pcd": compare_out, "distance_points": m_points, "distance_bytes": m_bytes})
        if normals is not None:
            normals_out = normals_out or os.path.join(workdir, "DenseCloudNormals.pcd")
            _, without = dc.compute_normals(radius=normals, download=False)
            n_points, n_bytes = dc.save_pcd_normals(normals_out)
            extra.update({"normals_pcd": normals_out, "normals_points": n_points, "normals_bytes": n_bytes, "without_normal": without})
    finally:
        dc.close()
    return {"poses": len(r["tum"]), "scans": n_scans, "stats": stats, "points": points, "bytes": size, "pcd": out, "poses_file": poses, "dump": dump, **extra}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=10)
    ap.add_argument("--voxel", type=float, default=0.1, help="voxel_size [m]; 0 = keep every point")
    ap.add_argument("--min-range", type=float, default=0.5)
    ap.add_argument("--out", help="the PCD (default: in a temporary directory)")
    ap.add_argument("--normals", type=float, metavar="RADIUS", help="also write x y z normal_x normal_y normal_z curvature with this neighbourhood radius [m]")
    ap.add_argument("--normals-out", help="the seven-field PCD (default: beside the x y z file's default)")
    ap.add_argument("--outliers", nargs=2, type=float, metavar=("K", "MUL"),
                    help="statistical outlier removal before anything else is derived: mean distance to the K nearest points, threshold mean + MUL * stddev")
    ap.add_argument("--outlier-radius", type=float, help="reach of the neighbour search [m] (default: the --normals radius, else three voxels)")
    ap.add_argument("--clean-out", help="the x y z PCD of the cleaned store (default: beside the x y z file's default)")
    ap.add_argument("--carve", nargs="*", type=float, metavar="V",
                    help="remove moving objects by ray carving before anything else is derived; optional values: CELL [m], RHO [m], PASSES (defaults 0.2 0.1 2)")
    ap.add_argument("--intensity", action="store_true", help="an `intensity` field after z in every file (a reflectance per surface orientation of the synthetic scene)")
    ap.add_argument("--clusters", nargs=2, type=float, metavar=("RADIUS", "MIN_SIZE"),
                    help="after --carve and before --outliers: remove the Euclidean clusters (points at most RADIUS [m] apart are connected) of fewer than MIN_SIZE points")
    ap.add_argument("--clusters-out", help="the x y z label PCD of the store without its small clusters (default: beside the x y z file's default)")
    ap.add_argument("--carved-out", help="the x y z PCD of the carved store (default: beside the x y z file's default)")
    ap.add_argument("--compare", metavar="PATH", help="after --outliers and before --normals: compare the store with this reference cloud (a binary PCD with x y z fields)")
    ap.add_argument("--compare-max", type=float, default=1.0, help="reach of the nearest-point search [m] (a placeholder default)")
    ap.add_argument("--compare-tol", type=float, default=0.1, help="the distance up to which a point counts as confirmed [m] (a placeholder default)")
    ap.add_argument("--compare-out", help="the x y z distance PCD of the store (default: beside the x y z file's default)")
    ap.add_argument("--align", action="store_true", help="with --compare: align the reference to the store by ICP before the comparison")
    ap.add_argument("--align-metric", choices=("point", "plane"), default="point",
                    help="with --align: point to point, or point to plane on the store's normals (computed first, at --normals' radius or 0.3 m)")
    ap.add_argument("--compare-displace", metavar="DEG,M", help="with --compare: move the reference rows by this known rigid motion first")
    ap.add_argument("--occupancy", nargs="?", type=float, const=0.2, metavar="CELL",
                    help="after --carve, --clusters and --outliers: the occupancy map of the rays of the rows left in the store, cells of CELL [m] (default 0.2)")
    ap.add_argument("--occupancy-out", help="the x y z hits passes state PCD of the map (default: DenseCloudOccupancy.pcd beside the x y z file's default)")
    ap.add_argument("--occupancy-slice", nargs=2, type=float, metavar=("LO", "HI"), help="with --occupancy: project the cells between these heights [m] into map.pgm + map.yaml")
    ap.add_argument("--map-out", help="the .pgm of the 2-D map; the .yaml goes beside it (default: map.pgm beside the x y z file's default)")
    ap.add_argument("--occupancy-rays-out", help="with --occupancy: the rays the map was built from (the store's points and sensor origins) as an .npz")
    ap.add_argument("--mesh", nargs="?", type=float, const=0.2, metavar="CELL",
                    help="after --carve, --clusters and --outliers: the fused surface of the rays of the rows left in the store as DenseCloudMesh.ply, cells of CELL [m] (default 0.2)")
    ap.add_argument("--mesh-out", help="the PLY of the mesh (default: DenseCloudMesh.ply beside the x y z file's default)")
    ap.add_argument("--tsdf-out", help="with --mesh: the signed distance field as an x y z tsdf weight PCD")
    a = ap.parse_args()
    if a.tsdf_out and a.mesh is None:
        ap.error("--tsdf-out needs --mesh")
    if (a.occupancy_slice or a.occupancy_rays_out) and a.occupancy is None:
        ap.error("--occupancy-slice and --occupancy-rays-out need --occupancy")
    if (a.align or a.compare_displace) and a.compare is None:
        ap.error("--align and --compare-displace need --compare")
    displace = None
    if a.compare_displace is not None:
        try:
            displace = tuple(float(v) for v in a.compare_displace.split(","))
        except ValueError:
            displace = ()
        if len(displace) != 2:
            ap.error("--compare-displace takes DEG,M")
    carve = None
    if a.carve is not None:
        if len(a.carve) > 3:
            ap.error("--carve takes at most three values: CELL RHO PASSES")
        carve = DenseCarveConfig(**dict(zip(("cell_size", "rho", "min_passes"), a.carve)))
        carve.min_passes = int(carve.min_passes)
    r = run(a.scans, out=a.out, voxel_size=a.voxel, min_range=a.min_range, normals=a.normals, normals_out=a.normals_out, outliers=a.outliers,
            outlier_radius=a.outlier_radius, clean_out=a.clean_out, carve=carve, carved_out=a.carved_out, intensity=a.intensity, clusters=a.clusters, clusters_out=a.clusters_out,
            compare=a.compare, compare_max=a.compare_max, compare_tol=a.compare_tol, compare_out=a.compare_out, align=a.align, align_metric=a.align_metric, compare_displace=displace,
            occupancy=None if a.occupancy is None else DenseOccupancyConfig(cell_size=a.occupancy), occupancy_out=a.occupancy_out, occupancy_slice=a.occupancy_slice,
            map_out=a.map_out, occupancy_rays_out=a.occupancy_rays_out,
            mesh=None if a.mesh is None else DenseSurfaceConfig(cell_size=a.mesh, truncation=3.0 * a.mesh), mesh_out=a.mesh_out, tsdf_out=a.tsdf_out)
    print(f"{r['poses']} poses, {r['scans']} scans: " + "  ".join(f"{k} {v}" for k, v in r["stats"].items()))
    print(f"{r['pcd']}: {r['points']} points, {r['bytes']} bytes")
    if carve is not None:
        t = r["carve"]
        print(f"carve (cell {carve.cell_size:g} m, rho {carve.rho:g} m, passes {carve.min_passes}): " + "  ".join(f"{k} {v}" for k, v in t.items()))
        print(f"{r['carved_pcd']}: {r['carved_points']} points, {r['carved_bytes']} bytes")
    if a.clusters is not None:
        print(f"clusters (radius {a.clusters[0]:g} m, min_size {int(a.clusters[1])}): " + "  ".join(f"{k} {v}" for k, v in r["clusters"].items()))
        print(f"{r['clusters_pcd']}: {r['clusters_points']} points, {r['clusters_bytes']} bytes")
    if a.outliers is not None:
        o = r["outliers"]
        print(f"outliers (k {int(a.outliers[0])}, mul {a.outliers[1]:g}, radius {r['outlier_radius']:g} m): " + "  ".join(f"{k} {o[k]}" for k in ("rows", "isolated", "above_threshold", "inliers"))
              + f"  threshold {o['threshold_m']:.4f} m")
        print(f"{r['clean_pcd']}: {r['clean_points']} points, {r['clean_bytes']} bytes")
    if a.occupancy is not None:
        m = r["occupancy"]
        print(f"occupancy (cell {a.occupancy:g} m): " + "  ".join(f"{k} {v}" for k, v in m.items()))
        print(f"{r['occupancy_pcd']}: {m['cells']} cells")
        if a.occupancy_slice is not None:
            i = r["map"]
            print(f"{r['map_pgm']}: {i['width']} x {i['height']} pixels, occupied {i['occupied']}  free {i['free']}  unknown {i['unknown']}; {r['map_yaml']}")
    if a.mesh is not None:
        print(f"surface (cell {a.mesh:g} m, truncation {3.0 * a.mesh:g} m): " + "  ".join(f"{k} {v}" for k, v in r["surface"].items()))
        print(f"{r['mesh_ply']}: " + "  ".join(f"{k} {v}" for k, v in r["mesh"].items()))
        if a.tsdf_out:
            print(f"{r['tsdf_pcd']}: {r['surface']['cells']} cells")
    if a.align:
        al = r["align"]
        for k, h in enumerate(al["history"]):
            plane = f"  used {h['used']}  plane rms {h['plane_rms_m']:.6f} m  min pivot {h['min_pivot']:.3e}" if a.align_metric == "plane" else ""
            print(f"align iteration {k}: matched {h['matched']}  unmatched {h['unmatched']}  rms {h['rms_m']:.6f} m  shift {h['shift_m']:.3e} m  rotation {h['rotation_rad']:.3e} rad" + plane)
        print(f"align: stop {al['stop']} after {al['iterations']} iterations")
        rows = [al["transform"]] + ([inverse_motion(r["applied"])] if "applied" in r else [])
        for name, T in zip(("recovered", "inverse of the applied"), rows):
            print(f"align {name}: " + "  ".join(" ".join(f"{v:.6f}" for v in row) for row in T))
        if "applied" in r:
            print(f"align: largest entry difference {np.abs(rows[0] - rows[1]).max():.3e}")
    if a.compare is not None:
        m = r["compare"]
        print(f"compare (max_distance {a.compare_max:g} m, tolerance {a.compare_tol:g} m): " + "  ".join(f"{k} {m[k]}" for k in ("rows", "ref_rows", "ref_invalid"))
              + "  " + "  ".join(f"{k} {m['accuracy'][k]}" for k in ("matched", "unmatched", "within")) + f"  mean {m['accuracy']['mean_m']:.6f} m  rms {m['accuracy']['rms_m']:.6f} m"
              + f"  precision {m['precision']:.6f}  recall {m['recall']:.6f}  f_score {m['f_score']:.6f}")
        print(f"{r['distance_pcd']}: {r['distance_points']} points, {r['distance_bytes']} bytes")
    if a.normals is not None:
        print(f"{r['normals_pcd']}: {r['normals_points']} points, {r['normals_bytes']} bytes, {r['without_normal']} without a normal")
