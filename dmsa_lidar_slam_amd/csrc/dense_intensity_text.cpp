// dense_intensity_text.cpp — the host-only side of include/dmsa_dense_intensity.h: the field of a sensor's message that carries the intensity
// and the headers of the two binary PCD layouts with an intensity field.  No device, no context.
#include "../../include/dmsa_dense_intensity.h"

#include <cstdio>

extern "C" {

// recalled from the drivers' message layouts (include/dmsa_dense_intensity.h, I5): x y z and the reflectance as the fourth field, a float32
int dmsa_sensor_intensity_field(int32_t sensor, dmsa_pointcloud2_field* out) {
    if (!out || sensor < DMSA_SENSOR_HESAI || sensor > DMSA_SENSOR_LIVOX_NS) return DMSA_ERR_INVALID;
    out->index = 3, out->datatype = DMSA_FIELD_FLOAT32;
    return DMSA_OK;
}

// decided here (I7): the x y z header with a fourth field; width = n, height = 1, the identity viewpoint, the counts twelve digits wide
int dmsa_pcd_header_xyzi_binary(int64_t n, char* out, int32_t cap) {
    if (n < 0 || n >= 1000000000000ll || !out || cap < 1) return DMSA_ERR_INVALID;
    const int len = std::snprintf(out, (size_t)cap,
                                  "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
                                  "WIDTH %012lld\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %012lld\nDATA binary\n",
                                  (long long)n, (long long)n);
    if (len < 0 || len >= cap) return DMSA_ERR_INVALID;
    return len;
}

int dmsa_pcd_header_xyzi_normals_binary(int64_t n, char* out, int32_t cap) {
    if (n < 0 || n >= 1000000000000ll || !out || cap < 1) return DMSA_ERR_INVALID;
    const int len = std::snprintf(out, (size_t)cap,
                                  "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity normal_x normal_y normal_z curvature\n"
                                  "SIZE 4 4 4 4 4 4 4 4\nTYPE F F F F F F F F\nCOUNT 1 1 1 1 1 1 1 1\nWIDTH %012lld\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %012lld\n"
                                  "DATA binary\n",
                                  (long long)n, (long long)n);
    if (len < 0 || len >= cap) return DMSA_ERR_INVALID;
    return len;
}

}  // extern "C"
