/*
 * dmsa_dense_intensity.h — C ABI of an intensity per point of the dense cloud (include/dmsa_dense_cloud.h): the reflectance value every
 * supported PointCloud2 layout carries as its fourth field, read on the device, carried in the fourth float of a point row through every
 * stage, and written as a fourth field of the three binary PCD files.
 *
 * The reference never reads intensity (its only mentions are in its RViz configuration).  Like the rules of the dense cloud, the semantics
 * are DECIDED HERE, stated below, and tested against an independent numpy model (tests/dense_intensity_model.py).  Same conventions as
 * dmsa_hip.h (contexts, status codes, no CPU fallback).  An object on which the switch of I1 was not called does what it did: the same
 * kernels, w = 1, 12- and 28-byte rows, byte for byte.
 *
 * I1  THE SWITCH.  dmsa_dense_cloud_with_intensity is legal only before the first scan is added and while no file is open, like
 *     dmsa_dense_cloud_retain; otherwise DMSA_ERR_INVALID with the reason in dmsa_last_error.  Calling it twice is fine.
 *     dmsa_dense_cloud_has_intensity returns 1 or 0 (a null object: DMSA_ERR_INVALID).
 * I2  THE VALUE NEVER DECIDES ANYTHING.  Rules 1-7 of dmsa_dense_cloud.h, T1-T7, O1-O6 and N0-N4 do not look at it.  A NaN or infinite
 *     intensity drops no point and enters no counter.  The survivor of a voxel is still its first hit, so a voxel's intensity is the
 *     intensity of that hit: nothing is averaged.
 * I3  dmsa_dense_cloud_add_scan ON AN INTENSITY OBJECT.  The fourth float of every input row is the intensity, taken bit for bit; the fourth
 *     float of every xyz_out row is the survivor's intensity, instead of 1.
 * I4  THE FIELD DESCRIPTOR.  index points into field_offsets of the message; datatype is a constant of sensor_msgs/PointField: 1 INT8,
 *     2 UINT8, 3 INT16, 4 UINT16, 5 INT32, 6 UINT32, 7 FLOAT32, 8 FLOAT64.  Conversion to float: types 1-4 are exact; types 5, 6 and 8 are the
 *     C conversion under round-to-nearest-even, and a FLOAT64 beyond the float range gives +-inf; type 7 passes its bits through.  The read
 *     is byte-wise at field_offsets[index] of every point (fields are not aligned in general), little-endian.  DMSA_ERR_INVALID: index >=
 *     num_fields; a datatype outside 1..8; a field that reaches beyond point_step or data (and whatever dmsa_decode_pointcloud2 refuses in a
 *     message of a sensor that names no field of its own).  On that error nothing is entered, exactly as for a bad stamp field.
 * I5  ENTRY POINTS ON THE DESCRIPTOR.  dmsa_decode_pointcloud2_field is the stage call: n = height * width floats, decoded on the device.
 *     dmsa_dense_cloud_add_pointcloud2_field is the fused path: the same bytes out as dmsa_decode_pointcloud2, then
 *     dmsa_decode_pointcloud2_field into the fourth float of its rows, then dmsa_dense_cloud_add_scan -- and the decoded scan does not visit
 *     the host.  The plain dmsa_dense_cloud_add_pointcloud2 on an intensity object gives every point the intensity +0.0f, which is the w the
 *     decoder writes.  dmsa_dense_cloud_add_pointcloud2_field on an object without the switch returns DMSA_ERR_INVALID.
 *     dmsa_sensor_intensity_field is host only: DMSA_SENSOR_HESAI through DMSA_SENSOR_LIVOX_NS give field 3, FLOAT32 (`intensity`, or
 *     `reflectivity` on Livox).  These are the drivers' message layouts, RECALLED like the PCD headers, not read off the drivers' sources or
 *     a recording; a message that differs names its field itself.  DMSA_SENSOR_SICK and DMSA_SENSOR_UNKNOWN return DMSA_ERR_INVALID: the
 *     caller names the field.
 * I6  THE STORE.  The fourth float of a retained point row is the intensity; origins keep w = 1.  dmsa_dense_cloud_retained returns it.
 *     remove_transients and remove_outliers carry it with the row.  Moments, normals, k-NN means, flags and pass counts of an intensity
 *     object equal those of a twin object without the switch, bit for bit.
 * I7  THE FILES.  All binary; fields in this order (decided here; a PCD reader maps by name):
 *       the streaming file (open_pcd / close_pcd)   16-byte rows   FIELDS x y z intensity
 *       save_pcd_retained                           16-byte rows   FIELDS x y z intensity
 *       save_pcd_normals                            32-byte rows   FIELDS x y z intensity normal_x normal_y normal_z curvature
 *     Every field is SIZE 4, TYPE F, COUNT 1; the other header lines and the twelve-digit patched counts are those of the x y z headers.
 *     The two header calls are host only, with the arguments and the statuses of their x y z twins.
 */
#ifndef DMSA_DENSE_INTENSITY_H
#define DMSA_DENSE_INTENSITY_H

#include "dmsa_dense_cloud.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    DMSA_FIELD_INT8 = 1,
    DMSA_FIELD_UINT8 = 2,
    DMSA_FIELD_INT16 = 3,
    DMSA_FIELD_UINT16 = 4,
    DMSA_FIELD_INT32 = 5,
    DMSA_FIELD_UINT32 = 6,
    DMSA_FIELD_FLOAT32 = 7,
    DMSA_FIELD_FLOAT64 = 8
};

/* I4 */
typedef struct {
    uint32_t index;    /* into dmsa_pointcloud2.field_offsets                */
    uint32_t datatype; /* sensor_msgs/PointField: DMSA_FIELD_INT8 .. FLOAT64 */
} dmsa_pointcloud2_field;

/* I1 */
int dmsa_dense_cloud_with_intensity(dmsa_dense_cloud* dc);
int dmsa_dense_cloud_has_intensity(dmsa_dense_cloud* dc);

/* I4-I5: out receives height * width floats (it may be NULL for an empty message). */
int dmsa_decode_pointcloud2_field(dmsa_ctx* ctx, const dmsa_pointcloud2* msg, const dmsa_pointcloud2_field* field, float* out);
/* I5: the arguments of the plain call for a message, and the field; xyz_out rows are x y z intensity. */
int dmsa_dense_cloud_add_pointcloud2_field(dmsa_dense_cloud* dc, const dmsa_pointcloud2* msg, int32_t sensor, const dmsa_pointcloud2_field* field,
                                           float* xyz_out, int64_t cap, int64_t* kept, dmsa_dense_stats* call_stats);
/* I5, host only */
int dmsa_sensor_intensity_field(int32_t sensor, dmsa_pointcloud2_field* out);

/* I7, host only: at most cap bytes incl. the terminating 0; the length or a negative status (n < 0 or n >= 10^12: DMSA_ERR_INVALID). */
int dmsa_pcd_header_xyzi_binary(int64_t n, char* out, int32_t cap);
int dmsa_pcd_header_xyzi_normals_binary(int64_t n, char* out, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* DMSA_DENSE_INTENSITY_H */
