// dense_cloud_from_raw.cpp — "Generate Dense Point Cloud" without Python: every raw point of a recorded sequence placed along its saved
// trajectory and written as a binary PCD (include/dmsa_dense_cloud.h).
//
//   dense_cloud_from_raw <raw dump> <Poses.txt> <sensor> <out.pcd> [radius] [--min-range m] [--max-range m] [--time-offset s] [--max-pose-gap s] [--voxel m]
//                        [--outlier-k K] [--outlier-mul MUL] [--outlier-radius m] [--carve] [--carve-cell m] [--carve-rho m] [--carve-passes N]
//                        [--cluster-min N] [--cluster-max N] [--cluster-radius m] [--cluster-labels out.pcd] [--intensity [INDEX:TYPE]]
//                        [--compare ref.pcd] [--compare-max m] [--compare-tol m] [--compare-out dist.pcd] [--compare-keep near|far]
//                        [--compare-transform T.txt] [--align] [--align-iters N] [--align-stop-t m] [--align-stop-r rad] [--align-out T.txt]
//                        [--align-metric point|plane] [--occupancy out.pcd] [--occupancy-cell m] [--occupancy-min-state s]
//                        [--occupancy-map map.pgm --occupancy-z lo hi] [--mesh out.ply] [--surface-cell m] [--surface-trunc m]
//                        [--surface-min-weight n] [--tsdf-out vox.pcd]
//
// With a radius [m] the survivors are retained and <out.pcd> gets seven fields, x y z normal_x normal_y normal_z curvature
// (include/dmsa_dense_normals.h; needs --voxel, radius between one and 64 voxels).
// With --outlier-k and/or --outlier-mul (defaults 8 and 1.0) the survivors are retained and go through statistical outlier removal first
// (include/dmsa_dense_outliers.h; needs --voxel; the search radius is --outlier-radius, else the normals' radius, else three voxels): with a
// radius the seven-field file is that of the cleaned store, without one <out.pcd> is the x y z file of the cleaned store.
// With --carve (or any of --carve-cell, --carve-rho, --carve-passes; defaults 0.2, 0.1, 2) moving objects are removed before either
// (include/dmsa_dense_carve.h; needs --voxel): every retained point that at least N rays of other points pass straight through leaves the
// store.
// With --cluster-min N (or any of --cluster-max, --cluster-radius, --cluster-labels; defaults 50, no upper bound) the Euclidean clusters of
// fewer than N points -- or of more than --cluster-max -- leave the store after the carving (include/dmsa_dense_clusters.h; needs --voxel; two
// points are connected when at most --cluster-radius apart, else the normals' radius, else three voxels).  --cluster-labels out.pcd writes
// the store as it then stands with a `label` field, the cluster of every point.
// With --compare ref.pcd (a binary PCD with x y z fields, such as any file this program writes: include/dmsa_dense_compare.h, D8) the store is
// compared with that reference cloud after the outliers and before the normals (needs --voxel): nearest distances both ways up to
// --compare-max (default 1 m), precision, recall and f_score at --compare-tol (default 0.1 m; both defaults are placeholders from no recorded
// data).  --compare-out dist.pcd writes the store with a `distance` field; --compare-keep near|far then removes what the reference does not
// confirm, or what it does.
// --compare-transform T.txt gives the rigid alignment of the reference into the map frame (D0's T: twelve numbers, three rows of four).
// With --align (or any of --align-iters, --align-stop-t, --align-stop-r, --align-out; defaults 30, 1e-4 m, 1e-5 rad) that alignment is refined
// by ICP before the comparison (include/dmsa_dense_align.h), from --compare-transform if one is given, else from the identity, with
// --compare-max as the reach of the pairs; one line per iteration and the stop reason are printed, --align-out T.txt writes the result in
// the format --compare-transform reads.  --align-metric plane aligns by point to plane (include/dmsa_dense_align_plane.h) on the normals of
// the store as it then stands, which are computed first, at the normals' radius, else 0.3 m; its lines also give the pairs used, the rms
// along the normals and the smallest pivot.
// With --occupancy out.pcd the rays of the rows then left in the store -- after the carving, the clusters and the outliers, before everything
// else -- are walked into an occupancy map (include/dmsa_dense_occupancy.h; needs --voxel): every cell seen occupied, seen free or left unknown,
// written as x y z hits passes state, the cells of state >= --occupancy-min-state (default 0: all).  --occupancy-cell (default 0.2) is the edge
// of the cells.  --occupancy-map map.pgm with --occupancy-z lo hi projects the cells between the two heights into the map.pgm + map.yaml
// pair of the ROS map_server (the .yaml goes beside the .pgm).  Thinning and every removal take their rays with them: only the rows still in
// the store are evidence.
// With --mesh out.ply the same rays, at the same place in the order, are fused into a truncated signed distance field
// (include/dmsa_dense_surface.h; needs --voxel) with cells of --surface-cell (default 0.2) and a truncation of --surface-trunc (default 0.6), and
// its zero set over the cells of at least --surface-min-weight samples (default 2) is written as a binary PLY of triangles.  --tsdf-out vox.pcd
// writes the field itself as x y z tsdf weight.
// The stages compose in the order carve, clusters, outliers, occupancy, surface, align, compare, normals.
// With --intensity every file gets an `intensity` field after z (include/dmsa_dense_intensity.h): read from field INDEX of the messages, of
// sensor_msgs/PointField datatype TYPE (1..8, or int8 uint8 int16 uint16 int32 uint32 float32 float64).  The raw dump stores the fields' offsets
// but not their datatypes, so without INDEX:TYPE the field is the one dmsa_sensor_intensity_field names for <sensor> (none for sick and unknown).
//
// <raw dump>: the flat message dump of include/dmsa_raw_sequence.h (scripts/rosbag_to_raw.py writes one from a bag); <Poses.txt>: the TUM
// lines the run wrote; <sensor>: hesai | ouster | robosense | velodyne | livoxXYZRTLT_s | livoxXYZRTLT_ns | sick | unknown.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/dmsa_dense_cloud.h"
#include "../include/dmsa_dense_normals.h"
#include "../include/dmsa_dense_carve.h"
#include "../include/dmsa_dense_occupancy.h"
#include "../include/dmsa_dense_surface.h"
#include "../include/dmsa_dense_clusters.h"
#include "../include/dmsa_dense_compare.h"
#include "../include/dmsa_dense_align.h"
#include "../include/dmsa_dense_align_plane.h"
#include "../include/dmsa_dense_outliers.h"
#include "../include/dmsa_dense_intensity.h"
#include "../include/dmsa_raw_sequence.h"

static int usage() {
    std::fprintf(stderr, "usage: dense_cloud_from_raw <raw dump> <Poses.txt> <sensor> <out.pcd> [radius] [--min-range m] [--max-range m] [--time-offset s] "
                         "[--max-pose-gap s] [--voxel m] [--outlier-k K] [--outlier-mul MUL] [--outlier-radius m] [--carve] [--carve-cell m] [--carve-rho m] "
                         "[--carve-passes N] [--cluster-min N] [--cluster-max N] [--cluster-radius m] [--cluster-labels out.pcd] [--intensity [INDEX:TYPE]] "
                         "[--compare ref.pcd] [--compare-max m] [--compare-tol m] [--compare-out dist.pcd] [--compare-keep near|far] [--compare-transform T.txt] "
                         "[--align] [--align-iters N] [--align-stop-t m] [--align-stop-r rad] [--align-out T.txt] [--align-metric point|plane] [--occupancy out.pcd] "
                         "[--occupancy-cell m] [--occupancy-min-state s] [--occupancy-map map.pgm --occupancy-z lo hi] [--mesh out.ply] [--surface-cell m] "
                         "[--surface-trunc m] [--surface-min-weight n] [--tsdf-out vox.pcd]\n");
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 5) return usage();
    const char* names[] = {"hesai", "ouster", "robosense", "velodyne", "livoxXYZRTLT_s", "livoxXYZRTLT_ns", "sick", "unknown"};
    int sensor = -1;
    for (int k = 0; k < 8; ++k)
        if (std::strcmp(argv[3], names[k]) == 0) sensor = k;
    if (sensor < 0) {
        std::fprintf(stderr, "unknown sensor %s\n", argv[3]);
        return usage();
    }
    dmsa_dense_config cfg;
    dmsa_default_dense_config(&cfg);
    dmsa_dense_normals_config ncfg;
    dmsa_default_dense_normals_config(&ncfg);
    dmsa_dense_outlier_config ocfg;
    dmsa_default_dense_outlier_config(&ocfg);
    dmsa_dense_carve_config tcfg;
    dmsa_default_dense_carve_config(&tcfg);
    dmsa_dense_cluster_config kcfg;
    dmsa_default_dense_cluster_config(&kcfg);
    bool outliers = false, carve = false, clusters = false, intensity = false, field_named = false;
    dmsa_pointcloud2_field field{0, 0};
    float outlier_radius = 0.0f, cluster_radius = 0.0f;
    const char* labels_path = nullptr;
    dmsa_dense_compare_config mcfg;
    dmsa_default_dense_compare_config(&mcfg);
    const char *compare_path = nullptr, *distance_path = nullptr;
    bool compare_keep = false;
    dmsa_dense_align_config acfg;
    dmsa_default_dense_align_config(&acfg);
    const char *transform_path = nullptr, *align_out = nullptr;
    bool align = false, plane = false;
    dmsa_dense_occupancy_config gcfg;
    dmsa_default_dense_occupancy_config(&gcfg);
    const char *occupancy_path = nullptr, *map_path = nullptr;
    int32_t occupancy_min_state = 0;
    bool occupancy_z = false;
    float z_lo = 0.0f, z_hi = 0.0f;
    dmsa_dense_surface_config scfg;
    dmsa_default_dense_surface_config(&scfg);
    const char *mesh_path = nullptr, *tsdf_path = nullptr;
    const bool normals = argc > 5 && std::strncmp(argv[5], "--", 2) != 0;
    if (normals) ncfg.radius = (float)std::atof(argv[5]);
    for (int a = normals ? 6 : 5; a < argc; a += 2) {
        if (!std::strcmp(argv[a], "--carve")) {  // (the one flag without a value)
            carve = true, a -= 1;
            continue;
        }
        if (!std::strcmp(argv[a], "--align")) {  // (a flag without a value as well)
            align = true, a -= 1;
            continue;
        }
        if (!std::strcmp(argv[a], "--intensity")) {  // (its value is optional: INDEX:TYPE)
            intensity = true, a -= 1;
            const char* colon = a + 2 < argc ? std::strchr(argv[a + 2], ':') : nullptr;
            if (!colon || !std::strncmp(argv[a + 2], "--", 2)) continue;
            const char* types[] = {"", "int8", "uint8", "int16", "uint16", "int32", "uint32", "float32", "float64"};
            field.index = (uint32_t)std::atoi(argv[a + 2]), field.datatype = (uint32_t)std::atoi(colon + 1);
            for (uint32_t k = 1; k <= 8; ++k)
                if (!std::strcmp(colon + 1, types[k])) field.datatype = k;
            if (field.datatype < 1 || field.datatype > 8) return usage();
            field_named = true, a += 1;
            continue;
        }
        if (!std::strcmp(argv[a], "--occupancy-z")) {  // (the one option with two values)
            if (a + 2 >= argc) return usage();
            z_lo = (float)std::atof(argv[a + 1]), z_hi = (float)std::atof(argv[a + 2]), occupancy_z = true, a += 1;
            continue;
        }
        if (a + 1 >= argc) return usage();
        const double v = std::atof(argv[a + 1]);
        if (!std::strcmp(argv[a], "--min-range")) cfg.min_range = (float)v;
        else if (!std::strcmp(argv[a], "--max-range")) cfg.max_range = (float)v;
        else if (!std::strcmp(argv[a], "--time-offset")) cfg.time_offset = v;
        else if (!std::strcmp(argv[a], "--max-pose-gap")) cfg.max_pose_gap = v;
        else if (!std::strcmp(argv[a], "--voxel")) cfg.voxel_size = (float)v;
        else if (!std::strcmp(argv[a], "--outlier-k")) ocfg.k = (int32_t)v, outliers = true;
        else if (!std::strcmp(argv[a], "--outlier-mul")) ocfg.stddev_mul = (float)v, outliers = true;
        else if (!std::strcmp(argv[a], "--outlier-radius")) outlier_radius = (float)v, outliers = true;
        else if (!std::strcmp(argv[a], "--carve-cell")) tcfg.cell_size = (float)v, carve = true;
        else if (!std::strcmp(argv[a], "--carve-rho")) tcfg.rho = (float)v, carve = true;
        else if (!std::strcmp(argv[a], "--carve-passes")) tcfg.min_passes = (int32_t)v, carve = true;
        else if (!std::strcmp(argv[a], "--cluster-min")) kcfg.min_size = (int32_t)v, clusters = true;
        else if (!std::strcmp(argv[a], "--cluster-max")) kcfg.max_size = (int32_t)v, clusters = true;
        else if (!std::strcmp(argv[a], "--cluster-radius")) cluster_radius = (float)v, clusters = true;
        else if (!std::strcmp(argv[a], "--cluster-labels")) labels_path = argv[a + 1], clusters = true;
        else if (!std::strcmp(argv[a], "--occupancy")) occupancy_path = argv[a + 1];
        else if (!std::strcmp(argv[a], "--occupancy-cell")) gcfg.cell_size = (float)v;
        else if (!std::strcmp(argv[a], "--occupancy-min-state")) occupancy_min_state = (int32_t)v;
        else if (!std::strcmp(argv[a], "--occupancy-map")) map_path = argv[a + 1];
        else if (!std::strcmp(argv[a], "--mesh")) mesh_path = argv[a + 1];
        else if (!std::strcmp(argv[a], "--surface-cell")) scfg.cell_size = (float)v;
        else if (!std::strcmp(argv[a], "--surface-trunc")) scfg.truncation = (float)v;
        else if (!std::strcmp(argv[a], "--surface-min-weight")) scfg.min_weight = (int32_t)v;
        else if (!std::strcmp(argv[a], "--tsdf-out")) tsdf_path = argv[a + 1];
        else if (!std::strcmp(argv[a], "--compare")) compare_path = argv[a + 1];
        else if (!std::strcmp(argv[a], "--compare-max")) mcfg.max_distance = (float)v;
        else if (!std::strcmp(argv[a], "--compare-tol")) mcfg.tolerance = (float)v;
        else if (!std::strcmp(argv[a], "--compare-out")) distance_path = argv[a + 1];
        else if (!std::strcmp(argv[a], "--compare-keep") && (!std::strcmp(argv[a + 1], "near") || !std::strcmp(argv[a + 1], "far")))
            mcfg.keep = argv[a + 1][0] == 'n' ? DMSA_COMPARE_KEEP_NEAR : DMSA_COMPARE_KEEP_FAR, compare_keep = true;
        else if (!std::strcmp(argv[a], "--compare-transform")) transform_path = argv[a + 1];
        else if (!std::strcmp(argv[a], "--align-iters")) acfg.max_iterations = (int32_t)v, align = true;
        else if (!std::strcmp(argv[a], "--align-stop-t")) acfg.stop_translation = v, align = true;
        else if (!std::strcmp(argv[a], "--align-stop-r")) acfg.stop_rotation = v, align = true;
        else if (!std::strcmp(argv[a], "--align-out")) align_out = argv[a + 1], align = true;
        else if (!std::strcmp(argv[a], "--align-metric") && (!std::strcmp(argv[a + 1], "point") || !std::strcmp(argv[a + 1], "plane")))
            plane = argv[a + 1][1] == 'l', align = true;
        else return usage();
    }
    if ((distance_path || compare_keep || transform_path || align) && !compare_path) return usage();
    if ((map_path != nullptr) != occupancy_z || (map_path && !occupancy_path)) return usage();
    const bool occupancy = occupancy_path != nullptr;
    if (tsdf_path && !mesh_path) return usage();
    const bool surface = mesh_path != nullptr;
    acfg.max_distance = mcfg.max_distance;
    // (the same five fields; min_pairs is each metric's own default)
    dmsa_dense_align_plane_config pcfg;
    dmsa_default_dense_align_plane_config(&pcfg);
    pcfg.max_distance = acfg.max_distance, pcfg.max_iterations = acfg.max_iterations, pcfg.stop_translation = acfg.stop_translation, pcfg.stop_rotation = acfg.stop_rotation;
    ocfg.radius = outlier_radius > 0.0f ? outlier_radius : normals ? ncfg.radius : 3.0f * cfg.voxel_size;
    kcfg.radius = cluster_radius > 0.0f ? cluster_radius : normals ? ncfg.radius : 3.0f * cfg.voxel_size;
    const bool compare = compare_path != nullptr;
    const bool retain = normals || outliers || carve || clusters || compare || occupancy || surface;
    // the reference cloud, read before the GPU is asked for anything
    std::vector<float> reference;
    if (compare) {
        int64_t ref_rows = 0;
        int got = dmsa_pcd_xyz_info(compare_path, &ref_rows);
        if (got == DMSA_OK) reference.resize((size_t)std::max<int64_t>(ref_rows, 1) * 3), got = dmsa_pcd_xyz_read(compare_path, reference.data(), ref_rows, &ref_rows);
        if (got != DMSA_OK) {
            std::fprintf(stderr, "%s: %s\n", compare_path, dmsa_pcd_xyz_last_error());
            return 1;
        }
        reference.resize((size_t)ref_rows * 3);
    }
    double T[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (transform_path) {
        std::FILE* f = std::fopen(transform_path, "r");
        int got = 0;
        double extra = 0.0;
        while (f && got < 12 && std::fscanf(f, "%lf", &T[got]) == 1) ++got;
        const bool more = f && std::fscanf(f, "%lf", &extra) == 1;
        if (f) std::fclose(f);
        if (got != 12 || more) {
            std::fprintf(stderr, "%s: twelve numbers are expected (three rows of four)\n", transform_path);
            return 1;
        }
    }
    if (intensity && !field_named && dmsa_sensor_intensity_field(sensor, &field) != DMSA_OK) {
        std::fprintf(stderr, "--intensity: no known intensity field for sensor %s; name it as INDEX:TYPE\n", argv[3]);
        return 2;
    }
    // the trajectory
    std::string text;
    {
        std::FILE* f = std::fopen(argv[2], "rb");
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", argv[2]);
            return 1;
        }
        char chunk[1 << 16];
        for (size_t got; (got = std::fread(chunk, 1, sizeof(chunk), f)) > 0;) text.append(chunk, got);
        std::fclose(f);
    }
    int64_t n_p = 0;
    char why[128];
    dmsa_parse_tum_poses(text.data(), (int64_t)text.size(), nullptr, nullptr, nullptr, 0, &n_p, why, sizeof(why));  // the counting pass
    std::vector<double> stamps((size_t)n_p), pos((size_t)n_p * 3), quat((size_t)n_p * 4);
    if (dmsa_parse_tum_poses(text.data(), (int64_t)text.size(), stamps.data(), pos.data(), quat.data(), n_p, &n_p, why, sizeof(why)) != DMSA_OK) {
        std::fprintf(stderr, "%s: %s\n", argv[2], why);
        return 1;
    }
    dmsa_ctx* ctx = nullptr;
    if (dmsa_create(0, 0, &ctx) != DMSA_OK) {
        std::fprintf(stderr, "no usable GPU (there is no CPU fallback)\n");
        return 1;
    }
    dmsa_dense_cloud* dc = nullptr;
    dmsa_raw_reader* reader = nullptr;
    int rc = dmsa_dense_cloud_create(ctx, &cfg, stamps.data(), pos.data(), quat.data(), n_p, &dc);
    if (rc == DMSA_OK && dmsa_raw_open(argv[1], &reader) != DMSA_OK) {
        std::fprintf(stderr, "%s is not a raw dump\n", argv[1]);
        rc = DMSA_ERR_INVALID;
    }
    if (rc == DMSA_OK && intensity) rc = dmsa_dense_cloud_with_intensity(dc);
    if (rc == DMSA_OK) rc = retain ? dmsa_dense_cloud_retain(dc) : dmsa_dense_cloud_open_pcd(dc, argv[4]);
    int64_t scans = 0, points = 0, bytes = 0;
    const auto t0 = std::chrono::steady_clock::now();
    while (rc == DMSA_OK) {
        int32_t type = 0;
        dmsa_pointcloud2 msg;
        dmsa_raw_imu imu;
        const int got = dmsa_raw_next(reader, &type, &msg, &imu);
        if (got == DMSA_RAW_END) break;
        if (got != DMSA_OK) {
            std::fprintf(stderr, "%s: truncated or malformed dump\n", argv[1]);
            rc = got;
            break;
        }
        if (type != DMSA_RAW_POINTCLOUD2) continue;
        int64_t kept = 0;
        rc = intensity ? dmsa_dense_cloud_add_pointcloud2_field(dc, &msg, sensor, &field, nullptr, 0, &kept, nullptr)
                       : dmsa_dense_cloud_add_pointcloud2(dc, &msg, sensor, nullptr, 0, &kept, nullptr);
        ++scans;
    }
    int64_t without = 0;
    dmsa_dense_outlier_stats ost{};
    dmsa_dense_carve_stats tst{};
    dmsa_dense_cluster_stats kst{};
    int64_t label_points = 0, label_bytes = 0;
    if (rc == DMSA_OK && carve) rc = dmsa_dense_cloud_count_passes(dc, &tcfg, nullptr, &tst);
    if (rc == DMSA_OK && carve) rc = dmsa_dense_cloud_remove_transients(dc, nullptr);
    if (rc == DMSA_OK && clusters) rc = dmsa_dense_cloud_classify_clusters(dc, &kcfg, nullptr, &kst);
    if (rc == DMSA_OK && clusters) rc = dmsa_dense_cloud_remove_clusters(dc, nullptr);
    if (rc == DMSA_OK && labels_path) rc = dmsa_dense_cloud_cluster_labels(dc, &kcfg, nullptr, nullptr);  // of the cleaned store: the labels of the file
    if (rc == DMSA_OK && labels_path) rc = dmsa_dense_cloud_save_pcd_labels(dc, labels_path, &label_points, &label_bytes);
    if (rc == DMSA_OK && outliers) rc = dmsa_dense_cloud_classify_outliers(dc, &ocfg, nullptr, &ost);
    if (rc == DMSA_OK && outliers) rc = dmsa_dense_cloud_remove_outliers(dc, nullptr);
    dmsa_dense_occupancy_stats gst{};
    dmsa_dense_occupancy_slice_info ginfo{};
    int64_t occupancy_rows = 0;
    std::string yaml_path;
    if (rc == DMSA_OK && occupancy) rc = dmsa_dense_cloud_build_occupancy(dc, &gcfg, &gst);
    if (rc == DMSA_OK && occupancy) rc = dmsa_dense_cloud_save_pcd_occupancy(dc, occupancy_path, occupancy_min_state, &occupancy_rows);
    if (rc == DMSA_OK && map_path) {
        yaml_path = map_path;
        const size_t dot = yaml_path.rfind('.'), slash = yaml_path.rfind('/');
        if (dot != std::string::npos && (slash == std::string::npos || dot > slash)) yaml_path.erase(dot);
        yaml_path += ".yaml";
        rc = dmsa_dense_cloud_occupancy_slice(dc, z_lo, z_hi, &ginfo, nullptr, 0);
        if (rc == DMSA_OK) rc = dmsa_dense_cloud_save_occupancy_map(dc, map_path, yaml_path.c_str(), z_lo, z_hi);
    }
    dmsa_dense_surface_stats sst{};
    dmsa_dense_mesh_stats fst{};
    if (rc == DMSA_OK && surface) rc = dmsa_dense_cloud_build_surface(dc, &scfg, &sst);
    if (rc == DMSA_OK && tsdf_path) rc = dmsa_dense_cloud_save_pcd_tsdf(dc, tsdf_path, nullptr);
    if (rc == DMSA_OK && surface) rc = dmsa_dense_cloud_extract_mesh(dc, scfg.min_weight, &fst);
    if (rc == DMSA_OK && surface) rc = dmsa_dense_cloud_save_ply_mesh(dc, mesh_path);
    dmsa_dense_compare_stats mst{};
    int64_t distance_points = 0, distance_bytes = 0, compare_left = 0;
    dmsa_dense_align_report arep{};
    dmsa_dense_align_plane_report prep{};
    if (rc == DMSA_OK && align && plane) rc = dmsa_dense_cloud_compute_normals(dc, &ncfg, nullptr, nullptr, nullptr);  // P0: of the store as it now stands
    if (rc == DMSA_OK && align && plane)
        rc = dmsa_dense_cloud_align_reference_plane(dc, reference.data(), (int64_t)(reference.size() / 3), 3, transform_path ? T : nullptr, &pcfg, T, &prep);
    if (rc == DMSA_OK && align && !plane)
        rc = dmsa_dense_cloud_align_reference(dc, reference.data(), (int64_t)(reference.size() / 3), 3, transform_path ? T : nullptr, &acfg, T, &arep);
    if (rc == DMSA_OK && align && align_out) {
        std::FILE* f = std::fopen(align_out, "w");
        bool ok = f != nullptr;
        for (int r = 0; ok && r < 3; ++r) ok = std::fprintf(f, "%.17g %.17g %.17g %.17g\n", T[4 * r], T[4 * r + 1], T[4 * r + 2], T[4 * r + 3]) > 0;
        if (f && std::fclose(f) != 0) ok = false;
        if (!ok) {
            std::fprintf(stderr, "cannot write %s\n", align_out);
            rc = DMSA_ERR_INVALID;
        }
    }
    // (after an alignment the object holds the reference as set_reference with the result would have left it: include/dmsa_dense_align.h, A7)
    if (rc == DMSA_OK && compare && !align)
        rc = dmsa_dense_cloud_set_reference(dc, reference.data(), (int64_t)(reference.size() / 3), 3, transform_path ? T : nullptr);
    if (rc == DMSA_OK && compare) rc = dmsa_dense_cloud_compare(dc, &mcfg, &mst);
    if (rc == DMSA_OK && distance_path) rc = dmsa_dense_cloud_save_pcd_distance(dc, distance_path, &distance_points, &distance_bytes);
    if (rc == DMSA_OK && compare_keep) rc = dmsa_dense_cloud_classify_by_reference(dc, &mcfg, nullptr, nullptr);
    if (rc == DMSA_OK && compare_keep) rc = dmsa_dense_cloud_remove_by_reference(dc, &compare_left);
    if (rc == DMSA_OK && normals) rc = dmsa_dense_cloud_compute_normals(dc, &ncfg, nullptr, nullptr, &without);
    if (rc == DMSA_OK)
        rc = normals ? dmsa_dense_cloud_save_pcd_normals(dc, argv[4], &points, &bytes)
             : outliers || carve || clusters || compare || occupancy || surface ? dmsa_dense_cloud_save_pcd_retained(dc, argv[4], &points, &bytes)
                        : dmsa_dense_cloud_close_pcd(dc, &points, &bytes);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc != DMSA_OK) std::fprintf(stderr, "failed with status %d: %s\n", rc, dmsa_last_error(ctx));
    dmsa_dense_stats st{};
    if (dc) dmsa_dense_cloud_stats(dc, &st);
    std::printf("poses %lld  scans %lld  points_in %lld  kept %lld  non_finite %lld  out_of_range %lld  out_of_time %lld  in_gap %lld  out_of_grid %lld  thinned %lld\n",
                (long long)n_p, (long long)scans, (long long)st.points_in, (long long)st.kept, (long long)st.non_finite, (long long)st.out_of_range,
                (long long)st.out_of_time, (long long)st.in_gap, (long long)st.out_of_grid, (long long)st.thinned);
    if (rc == DMSA_OK)
        std::printf("%s: %lld points, %lld bytes; %.3f s, %.3g points/s in\n", argv[4], (long long)points, (long long)bytes, sec, sec > 0 ? st.points_in / sec : 0.0);
    if (rc == DMSA_OK && carve)
        std::printf("carve: cell %g m, rho %g m, passes %d: rows %lld  rays_walked %lld  rays_skipped %lld  cells_traversed %lld  pair_tests %lld  seen_through %lld  "
                    "transient %lld  kept %lld\n", (double)tcfg.cell_size, (double)tcfg.rho, (int)tcfg.min_passes, (long long)tst.rows, (long long)tst.rays_walked,
                    (long long)tst.rays_skipped, (long long)tst.cells_traversed, (long long)tst.pair_tests, (long long)tst.seen_through, (long long)tst.transient,
                    (long long)tst.kept);
    if (rc == DMSA_OK && clusters)
        std::printf("clusters: radius %g m, min_size %d, max_size %d: rows %lld  clusters %lld  largest %lld  kept_rows %lld  kept_clusters %lld  small_rows %lld  "
                    "large_rows %lld\n", (double)kcfg.radius, (int)kcfg.min_size, (int)kcfg.max_size, (long long)kst.rows, (long long)kst.clusters, (long long)kst.largest,
                    (long long)kst.kept_rows, (long long)kst.kept_clusters, (long long)kst.small_rows, (long long)kst.large_rows);
    if (rc == DMSA_OK && labels_path) std::printf("%s: %lld points, %lld bytes\n", labels_path, (long long)label_points, (long long)label_bytes);
    if (rc == DMSA_OK && occupancy)
        std::printf("occupancy: cell %g m: rows %lld  rays_walked %lld  rays_skipped %lld  cells_traversed %lld  cells_out_of_range %lld  cells %lld  occupied %lld  "
                    "free %lld  unknown %lld  table_slots %lld  table_builds %lld\n%s: %lld cells of state >= %d\n", (double)gcfg.cell_size, (long long)gst.rows,
                    (long long)gst.rays_walked, (long long)gst.rays_skipped, (long long)gst.cells_traversed, (long long)gst.cells_out_of_range, (long long)gst.cells,
                    (long long)gst.occupied, (long long)gst.free, (long long)gst.unknown, (long long)gst.table_slots, (long long)gst.table_builds, occupancy_path,
                    (long long)occupancy_rows, (int)occupancy_min_state);
    if (rc == DMSA_OK && map_path)
        std::printf("%s: %d x %d pixels, occupied %lld  free %lld  unknown %lld; %s\n", map_path, (int)ginfo.width, (int)ginfo.height, (long long)ginfo.occupied,
                    (long long)ginfo.free, (long long)ginfo.unknown, yaml_path.c_str());
    if (rc == DMSA_OK && surface)
        std::printf("surface: cell %g m, truncation %g m: rows %lld  rays_walked %lld  rays_skipped %lld  cells_traversed %lld  cells_out_of_range %lld  cells %lld  "
                    "cells_valid %lld  table_slots %lld  table_builds %lld\n%s: min_weight %d: tetrahedra_meshed %lld  vertices %lld  triangles %lld\n",
                    (double)scfg.cell_size, (double)scfg.truncation, (long long)sst.rows, (long long)sst.rays_walked, (long long)sst.rays_skipped,
                    (long long)sst.cells_traversed, (long long)sst.cells_out_of_range, (long long)sst.cells, (long long)sst.cells_valid, (long long)sst.table_slots,
                    (long long)sst.table_builds, mesh_path, (int)scfg.min_weight, (long long)fst.tetrahedra_meshed, (long long)fst.vertices, (long long)fst.triangles);
    if (rc == DMSA_OK && tsdf_path) std::printf("%s: %lld cells\n", tsdf_path, (long long)sst.cells);
    if (rc == DMSA_OK && outliers)
        std::printf("outliers: k %d, mul %g, radius %g m: rows %lld  isolated %lld  above_threshold %lld  inliers %lld  threshold %.4f m\n", (int)ocfg.k,
                    (double)ocfg.stddev_mul, (double)ocfg.radius, (long long)ost.rows, (long long)ost.isolated, (long long)ost.above_threshold, (long long)ost.inliers,
                    ost.threshold_m);
    if (rc == DMSA_OK && align) {
        const char* stops[] = {"CONVERGED", "MAX_ITERATIONS", "TOO_FEW_PAIRS", "DEGENERATE"};
        for (int k = 0; !plane && k < arep.iterations; ++k) {
            const dmsa_dense_align_iteration& it = arep.history[k];
            std::printf("align: iteration %d  matched %lld  unmatched %lld  rms %.6f m  shift %.3e m  rotation %.3e rad\n", k, (long long)it.matched, (long long)it.unmatched,
                        it.rms_m, it.shift_m, it.rotation_rad);
        }
        for (int k = 0; plane && k < prep.iterations; ++k) {
            const dmsa_dense_align_plane_iteration& it = prep.history[k];
            std::printf("align: iteration %d  matched %lld  unmatched %lld  rms %.6f m  shift %.3e m  rotation %.3e rad  used %lld  plane rms %.6f m  min pivot %.3e\n", k,
                        (long long)it.matched, (long long)it.unmatched, it.rms_m, it.shift_m, it.rotation_rad, (long long)it.used, it.plane_rms_m, it.min_pivot);
        }
        std::printf("align: max_distance %g m: stop %s after %d iterations\n", (double)acfg.max_distance, stops[plane ? prep.stop : arep.stop],
                    (int)(plane ? prep.iterations : arep.iterations));
        for (int r = 0; r < 3; ++r) std::printf("align: T %.9f %.9f %.9f %.9f\n", T[4 * r], T[4 * r + 1], T[4 * r + 2], T[4 * r + 3]);
        if (align_out) std::printf("%s: the transform\n", align_out);
    }
    if (rc == DMSA_OK && compare) {
        const dmsa_dense_compare_direction &ac = mst.accuracy, &co = mst.completeness;
        std::printf("compare: max_distance %g m, tolerance %g m: rows %lld  ref_rows %lld  ref_invalid %lld  matched %lld  unmatched %lld  within %lld  mean %.6f m  "
                    "rms %.6f m  ref_matched %lld  ref_unmatched %lld  ref_within %lld  ref_mean %.6f m  ref_rms %.6f m  precision %.6f  recall %.6f  f_score %.6f\n",
                    (double)mcfg.max_distance, (double)mcfg.tolerance, (long long)mst.rows, (long long)mst.ref_rows, (long long)mst.ref_invalid, (long long)ac.matched,
                    (long long)ac.unmatched, (long long)ac.within, ac.mean_m, ac.rms_m, (long long)co.matched, (long long)co.unmatched, (long long)co.within, co.mean_m,
                    co.rms_m, mst.precision, mst.recall, mst.f_score);
    }
    if (rc == DMSA_OK && distance_path) std::printf("%s: %lld points, %lld bytes\n", distance_path, (long long)distance_points, (long long)distance_bytes);
    if (rc == DMSA_OK && compare_keep) std::printf("compare: keep %s: %lld rows left\n", mcfg.keep == DMSA_COMPARE_KEEP_NEAR ? "near" : "far", (long long)compare_left);
    if (rc == DMSA_OK && intensity) std::printf("intensity: field %u, datatype %u\n", (unsigned)field.index, (unsigned)field.datatype);
    if (rc == DMSA_OK && normals) std::printf("normals: radius %g m, %lld points without one\n", (double)ncfg.radius, (long long)without);
    if (reader) dmsa_raw_close(reader);
    dmsa_dense_cloud_destroy(dc);
    dmsa_destroy(ctx);
    return rc == DMSA_OK ? 0 : 1;
}
