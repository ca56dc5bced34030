/*
 * dmsa_wire_formats.h — C ABI of the data formats either side of the path: the per-sensor
 * sensor_msgs/PointCloud2 decoding of the node and the two files it writes, the TUM pose lines of Poses.txt and the ASCII PointCloud.pcd.
 *
 *   dmsa_slam_ros::callbackPointCloud   src/dmsa_slam_ros.cpp:374-486        (PointCloud2 bytes -> PointStampId)
 *   OutputManagement::addPoseToFile     include/DMSA/OutputManagement.h:80-96 (TUM line)
 *   OutputManagement::saveDensePoses    include/DMSA/OutputManagement.h:98-171 (non-keyframe pose composition :148-153, :176-182)
 *   io::savePCDFileASCII(filename, KeyframeMap.globalPoints)   src/dmsa_slam_ros.cpp:286-291, :495-506 (PointCloud.pcd)
 *
 * rosbag / ROS message transport itself needs ROS (absent): the decoder takes the message's byte blob and the few header fields
 * it reads.  Decoding is byte work, one point per thread on the device.  The pose text (one line per pose) and the PCD header are host
 * work; the PCD rows -- seven exactly rounded "%.8g" conversions per map point, millions of points per save -- are formatted on the device
 * (csrc/pcd_kernels.hip), chunk by chunk, while the host writes the previous chunk.
 *
 * PCL is not part of the reference tree and was not at hand when this was written: the header text, the refusal of an empty cloud and the row
 * rules (precision 8 in the classic locale, `nan` for every NaN, padding words not written) are RECALLED from PCL 1.10's io/pcd_io
 * (PCDWriter::generateHeader / writeASCII), not read off its source.  What the rows are tested against is C's printf("%.8g").
 */
#ifndef DMSA_WIRE_FORMATS_H
#define DMSA_WIRE_FORMATS_H

#include "dmsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* config.sensor (dmsa_slam_ros.cpp:411-481) */
enum {
    DMSA_SENSOR_HESAI = 0,         /* stamp f64 @fields[4], ring u16 @fields[5]                                  (:411-419) */
    DMSA_SENSOR_OUSTER = 1,        /* t u32 ns @fields[4] relative to the header stamp, ring u8 @fields[6]       (:420-430) */
    DMSA_SENSOR_ROBOSENSE = 2,     /* ring u16 @fields[4], stamp f64 @fields[5]                                  (:431-439) */
    DMSA_SENSOR_VELODYNE = 3,      /* ring u16 @fields[4], time f32 @fields[5] relative to the header stamp      (:440-448) */
    DMSA_SENSOR_LIVOX_S = 4,       /* stamp f64 @fields[6] in seconds, id = k % 1000                             (:449-458) */
    DMSA_SENSOR_LIVOX_NS = 5,      /* stamp f64 @fields[6] in nanoseconds (1e-9 * value), id = k % 1000          (:459-469) */
    DMSA_SENSOR_SICK = 6,          /* time f32 @fields[8] relative to the header stamp, ring i8 @fields[11]      (:470-478) */
    DMSA_SENSOR_UNKNOWN = 7        /* stamp = header + deltaT * k / n, id = k % 1000                             (:479-486) */
};

/* The parts of a sensor_msgs/PointCloud2 the callback reads. */
typedef struct dmsa_pointcloud2 {
    uint32_t        height, width;   /* n = height * width points                                                        */
    uint32_t        point_step;      /* bytes per point                                                                  */
    uint32_t        num_fields;
    const uint32_t* field_offsets;   /* msg->fields[i].offset; fields 0..2 are x, y, z (float32)                         */
    const uint8_t*  data;            /* msg->data                                                                        */
    uint64_t        data_bytes;
    double          stamp_msg;       /* msg->header.stamp.toSec()                                                        */
    double          delta_t_pcs;     /* stampMsg - lastPcMsgStamp (:394), read by DMSA_SENSOR_UNKNOWN only               */
} dmsa_pointcloud2;

/* == the loop of callbackPointCloud (:399-486).  xyz_out n x 4 floats (w = 0: PointStampId is value-initialised, preProcess sets it
 * to 1 later), stamp_out n doubles (PointStampId::stamp), id_out n (PointStampId::id); isStatic = 0 for every point.
 * DMSA_ERR_INVALID when the sensor needs a field the message does not have or a field reaches beyond point_step / data. */
int dmsa_decode_pointcloud2(dmsa_ctx* ctx, const dmsa_pointcloud2* msg, int32_t sensor, float* xyz_out, double* stamp_out, int32_t* id_out);

/* == addPoseToFile (OutputManagement.h:80-96): "stamp tx ty tz qx qy qz qw\n" with 6 / 5 / 6 fixed decimals, the quaternion from
 * Eigen's Quaterniond(axang2rotm(orient)).  Writes at most cap bytes incl. the terminating 0; returns the line length (without the
 * 0) or a negative status. */
int dmsa_format_tum_pose(double stamp, const double pos[3], const double orient[3], char* out, int32_t cap);

/* == the non-keyframe pose composition of saveDensePoses / makeNonKeyframePoseGlobal (:148-153, :176-182):
 * pos_out = R(key_orient) * rel_transl + key_pos, orient_out = rotm2axang(R(key_orient) * R(rel_orient)). */
int dmsa_compose_nonkeyframe_pose(const double key_pos[3], const double key_orient[3], const double rel_transl[3], const double rel_orient[3],
                                  double pos_out[3], double orient_out[3]);

/* ---- PointCloud.pcd: pcl::io::savePCDFileASCII of a PointCloud<PointNormal> (precision 8) ------------------------------------------ */
/* The header for width = n, height = 1: eleven lines, "# .PCD v0.7 - Point Cloud Data file format" .. "DATA ascii", each ending in '\n'.
 * Host-only, no context.  Writes at most cap bytes incl. the terminating 0; returns the length (without the 0) or a negative status. */
int dmsa_pcd_header_pointnormal(int64_t n, char* out, int32_t cap);

/* n rows "x y z normal_x normal_y normal_z curvature\n" (single spaces, no leading or trailing space; the fourth float of a point or a normal
 * is not written).  Every finite value prints as printf("%.8g", (double)v) -- exactly rounded, at most 14 characters, so a row has at most 105
 * bytes --, any NaN as "nan", infinities as "inf" / "-inf".
 *   xyz        n x 4 host floats, or NULL = rows first .. first + n - 1 of the resident global points (dmsa_get_global_points)
 *   normal     n x 4 host floats, or NULL = the same rows of the resident global normals (dmsa_get_global_normals: keyframe model only)
 *   curvature  n host floats, or NULL = 0 for every row, which is what the reference's file holds: MapManagement::addKeyframe value-initialises
 *              globalPoints (MapManagement.h:369) and updateGlobalPoints (:142-144) writes xyz and normals only.
 * `first` counts rows of the RESIDENT arrays; a host array holds the n rows of the call themselves.  out: cap bytes, no terminating 0;
 * *bytes_out = the bytes the rows take.  A capacity too small gives DMSA_ERR_INVALID with *bytes_out still set (as dmsa_select_static_points
 * reports its count).  All arguments are checked before anything is launched. */
int dmsa_format_pcd_rows(dmsa_ctx* ctx, const float* xyz, const float* normal, const float* curvature, int64_t first, int64_t n, char* out, int64_t cap,
                         int64_t* bytes_out);

/* The whole file: header + all n rows (sources as above, first = 0) written to `path`.  The rows are formatted in chunks of 2^18 rows into two
 * device buffers and copied back into two pinned host buffers on a second stream: the host writes chunk i - 1 while chunk i is copied back and
 * chunk i + 1 is formatted, and the memory for text is bounded by the chunk, not by the map.  n == 0 is DMSA_ERR_INVALID and writes no file
 * (PCL refuses an empty cloud); a path that cannot be opened or written gives a negative status and the reason in dmsa_last_error.
 * *bytes_written = the size of the file. */
int dmsa_save_pcd_ascii(dmsa_ctx* ctx, const char* path, const float* xyz, const float* normal, const float* curvature, int64_t n, int64_t* bytes_written);
/* The same with the chunk size in rows (<= 0: the default; at most 2^24, so that the row offsets of a chunk fit an int32): tests run the chunk edges
 * with small chunks. */
int dmsa_save_pcd_ascii_ex(dmsa_ctx* ctx, const char* path, const float* xyz, const float* normal, const float* curvature, int64_t n, int64_t chunk_rows,
                           int64_t* bytes_written);

#ifdef __cplusplus
}
#endif
#endif /* DMSA_WIRE_FORMATS_H */
