/*
 * dmsa_dense_cloud.h — C ABI of the step AFTER the run: the dense point cloud.  Every raw point of every scan is placed at the pose
 * interpolated for its own time stamp along a saved trajectory (the stamp tx ty tz qx qy qz qw lines of Poses.txt), gated, thinned to one
 * point per voxel across all scans, and written as a binary PCD.
 *
 * The reference's README ends with "Generate Dense Point Cloud" and hands this step to a companion program that is not part of the
 * reference tree and was not at hand: nothing here is a restatement of its code.  The semantics are DECIDED HERE, stated below, and tested
 * against an independent numpy / scipy model (tests/dense_cloud_model.py).
 *
 * Same conventions as dmsa_hip.h (contexts, status codes, float[n][4] points, no CPU fallback).
 *
 * TRAJECTORY  n_p >= 2 poses of the IMU frame in the world (what Poses.txt holds): stamps s_k strictly increasing doubles, positions
 * double[3], unit quaternions in (x, y, z, w) order as in a TUM line, normalised on the host in double (q / sqrt(x*x + y*y + z*z + w*w)).
 * A zero or non-finite quaternion, a non-finite stamp or position, or stamps that do not increase give DMSA_ERR_INVALID.
 *
 * PER POINT i of a scan: raw sensor-frame x, y, z (float) and stamp t_i (double), as dmsa_decode_pointcloud2 delivers them.  A point fails
 * at the FIRST rule below that it breaks:
 *   1. non-finite coordinates or stamp                                                                      -> non_finite
 *   2. range r = sqrtf(x*x + (y*y + z*z)) (the expression of DmsaSlam::preProcess as this library evaluates it); kept iff
 *      r > min_range and (max_range <= 0 or r < max_range) -- the strictness of DmsaSlam.h:616                -> out_of_range
 *   3. t = t_i + time_offset; kept iff s_0 <= t <= s_{n_p-1}                                                  -> out_of_time
 *      segment j = the largest index with s_j <= t, capped at n_p - 2 (t == s_{n_p-1} is segment n_p - 2 with u = 1);
 *      u = (t - s_j) / (s_{j+1} - s_j);
 *      max_pose_gap > 0 and s_{j+1} - s_j > max_pose_gap: lost tracking is not interpolated across            -> in_gap
 *   4. pose at t in fp64, every operation rounded on its own (no fused multiply-add): the axis-angle o = slerp(q_j, q_{j+1}, u) and
 *      R = exp(o) of the window's dense pose tables (csrc/k1_pose_math.h: d_slerp_quat, d_so3_exp, on include/dmsa_detmath.h);
 *      tr = p_j + u * (p_{j+1} - p_j) per axis
 *   5. in float: p_imu = lidar_to_imu * (x, y, z, 1), g = [(float)R | (float)tr] * (p_imu, 1), each row as ((c0*x + c1*y) + c2*z) + c3
 *   6. voxel_size > 0: c_a = floorf(g_a / voxel_size) per axis (an IEEE float division); a c_a outside [-2^20, 2^20)  -> out_of_grid
 *      the voxel key is the three cells biased by 2^20, 21 bits each.  A point is kept iff no point of an EARLIER SCAN (call order) and no
 *      point with a LOWER INDEX in its own scan that passed rules 1-5 (and the grid bound) fell in the same voxel     -> thinned
 *      -- a rule that does not depend on the order in which threads run.
 *   7. survivors are written in input order (stable); scans follow in call order.
 */
#ifndef DMSA_DENSE_CLOUD_H
#define DMSA_DENSE_CLOUD_H

#include "dmsa_wire_formats.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmsa_dense_config {
    float  lidar_to_imu[16];  /* identity; column-major as in dmsa_preprocess_config: Config.h:58        */
    float  min_range;         /* 0:   points at or below this range are dropped                          */
    float  max_range;         /* 0:   <= 0 = no upper gate                                               */
    double time_offset;       /* 0:   added to every point stamp before it meets the trajectory          */
    double max_pose_gap;      /* 0:   <= 0 = every segment is interpolated across                        */
    float  voxel_size;        /* 0:   <= 0 = no thinning                                                 */
    int32_t pad;
} dmsa_dense_config;
void dmsa_default_dense_config(dmsa_dense_config* cfg);

/* where the points of a call (or of all calls so far) went: points_in = kept + the six drop counters */
typedef struct dmsa_dense_stats {
    int64_t points_in;
    int64_t kept;
    int64_t non_finite;
    int64_t out_of_range;
    int64_t out_of_time;
    int64_t in_gap;
    int64_t out_of_grid;
    int64_t thinned;
} dmsa_dense_stats;

typedef struct dmsa_dense_cloud dmsa_dense_cloud;

/* The trajectory is checked, normalised and uploaded once.  The object uses the context's streams and error text (dmsa_last_error) and
 * must be destroyed before the context.  max_range, min_range, voxel_size must not be NaN. */
int  dmsa_dense_cloud_create(dmsa_ctx* ctx, const dmsa_dense_config* cfg, const double* stamps, const double* pos /* n_p x 3 */,
                             const double* quat_xyzw /* n_p x 4 */, int64_t n_p, dmsa_dense_cloud** out);
void dmsa_dense_cloud_destroy(dmsa_dense_cloud* dc); /* closes an open file without patching its counts */

/* The stage call of rules 3-4: the placing kernel's own device function run for n stamps t (taken as they are: time_offset is NOT added).
 * pose12_out: n x 12 doubles, R row-major then tr; segment_out: n, the segment j, or -1 out of time (a NaN stamp too) / -2 in gap -- the
 * twelve doubles of such a stamp are zero.  Either output may be NULL. */
int dmsa_dense_cloud_interpolate(dmsa_dense_cloud* dc, const double* t, int64_t n, double* pose12_out, int32_t* segment_out);

/* One scan through rules 1-7.  xyz n x 4 floats (the 4th is ignored), stamps n doubles.  xyz_out (cap x 4 floats, w = 1) may be NULL: the
 * survivors then go to the open file and the statistics only, and cap is not looked at.  *kept = survivors of this scan; call_stats
 * (optional) = this call's counters.  A capacity that is too small gives DMSA_ERR_INVALID with *kept (and call_stats) still set, as
 * dmsa_select_static_points reports its count; the scan is then NOT entered into the voxel set, the cumulative statistics or the file:
 * the next call gives what it would have given without this one (the table may have grown: more room, the same set).  DMSA_ERR_NOMEM: the voxel table could not take the scan (a probe ran out of its bound or the
 * table could not grow); nothing is written and the object is as before. */
int dmsa_dense_cloud_add_scan(dmsa_dense_cloud* dc, const float* xyz, const double* stamps, int64_t n, float* xyz_out, int64_t cap, int64_t* kept,
                              dmsa_dense_stats* call_stats);

/* The same for one sensor_msgs/PointCloud2 message: decoded on the device as dmsa_decode_pointcloud2 does it, with the same checks and the same
 * DMSA_ERR_INVALID, and placed without the decoded scan visiting the host.  Same bytes out as dmsa_decode_pointcloud2 followed by dmsa_dense_cloud_add_scan. */
int dmsa_dense_cloud_add_pointcloud2(dmsa_dense_cloud* dc, const dmsa_pointcloud2* msg, int32_t sensor, float* xyz_out, int64_t cap, int64_t* kept,
                                     dmsa_dense_stats* call_stats);

/* counters of all successful calls so far */
int dmsa_dense_cloud_stats(dmsa_dense_cloud* dc, dmsa_dense_stats* total);

/* The voxel set is an open-addressing table in HBM, 16 bytes per slot, a power-of-two number of slots, never more than half full: before a
 * scan of n points is launched the table is grown (and rehashed on the device) to at least 2 * (occupied + n) slots.
 * dmsa_dense_cloud_reserve sizes it up front for `points` more points; dmsa_dense_cloud_table_info reports slots and occupied voxels
 * (either pointer may be NULL). */
int dmsa_dense_cloud_reserve(dmsa_dense_cloud* dc, int64_t points);
int dmsa_dense_cloud_table_info(dmsa_dense_cloud* dc, int64_t* slots, int64_t* occupied);

/* ---- the file: a binary PCD of x y z ---------------------------------------------------------------------------------------------------
 * While a file is open, the survivors of every added scan are appended as 12-byte rows (x, y, z as little-endian floats): packed on the device,
 * copied back into two pinned buffers on the context's second stream, and written by the host while the next scan is processed.
 * The header -- RECALLED from PCL's description of the PCD v0.7 format, like the PointNormal header of dmsa_wire_formats.h, not read off
 * PCL's source -- is
 *   # .PCD v0.7 - Point Cloud Data file format | VERSION 0.7 | FIELDS x y z | SIZE 4 4 4 | TYPE F F F | COUNT 1 1 1 | WIDTH <n> | HEIGHT 1 |
 *   VIEWPOINT 0 0 0 1 0 0 0 | POINTS <n> | DATA binary
 * one line each; <n> is twelve zero-padded digits, so that close can patch WIDTH and POINTS in place.
 * dmsa_pcd_header_xyz_binary: host-only; writes at most cap bytes incl. the terminating 0; returns the length or a negative status
 * (n < 0 or n >= 10^12: DMSA_ERR_INVALID).
 * open: a path that cannot be opened gives DMSA_ERR_INVALID and the reason in dmsa_last_error; one file at a time.
 * close: *points / *bytes (optional) = rows in the file / its size.  Closing with zero points removes the file and returns DMSA_ERR_INVALID
 * (PCL refuses an empty cloud). */
int dmsa_pcd_header_xyz_binary(int64_t n, char* out, int32_t cap);
int dmsa_dense_cloud_open_pcd(dmsa_dense_cloud* dc, const char* path);
int dmsa_dense_cloud_close_pcd(dmsa_dense_cloud* dc, int64_t* points, int64_t* bytes);

/* Host only, no context: the inverse of dmsa_format_tum_pose for the lines "stamp tx ty tz qx qy qz qw" of `text` (bytes long, no
 * terminating 0 needed; '\n' or "\r\n" line ends).  Blank lines and lines whose first non-blank character is '#' are skipped.  stamps
 * (cap), pos (cap x 3), quat_xyzw (cap x 4) receive the first cap poses (they may be NULL with cap = 0: a counting pass); *n_out = the
 * number of pose lines.  More poses than cap: DMSA_ERR_INVALID with *n_out set.  A line that does not hold exactly eight numbers:
 * DMSA_ERR_INVALID, *n_out = the poses before it, and "line <1-based number>: ..." in err (err_cap bytes incl. the terminating 0; may be
 * NULL).  The quaternions are returned as written: dmsa_dense_cloud_create normalises. */
int dmsa_parse_tum_poses(const char* text, int64_t bytes, double* stamps, double* pos, double* quat_xyzw, int64_t cap, int64_t* n_out, char* err,
                         int32_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* DMSA_DENSE_CLOUD_H */
