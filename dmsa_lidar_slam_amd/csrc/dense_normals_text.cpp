// dense_normals_text.cpp — the host-only side of include/dmsa_dense_normals.h: the defaults, N4 for one row through the header the device
// kernel compiles (csrc/pcl_eigen33.h), and the header of the seven-field binary PCD.  No device, no context.
#include "../../include/dmsa_dense_normals.h"

#include <cstdio>

#include "pcl_eigen33.h"

extern "C" {

void dmsa_default_dense_normals_config(dmsa_dense_normals_config* cfg) {
    if (!cfg) return;
    cfg->radius = 0.3f, cfg->min_neighbours = 5;
}

int dmsa_dense_normal_from_moments(const int64_t m[10], const float view[3], int32_t min_neighbours, float out[4]) {
    if (!m || !view || !out) return DMSA_ERR_INVALID;
    long long mm[10];
    for (int a = 0; a < 10; ++a) mm[a] = (long long)m[a];
    if (mm[0] < 0) return DMSA_ERR_INVALID;
    (void)dmsa::dense_normal_from_moments(mm, view[0], view[1], view[2], min_neighbours, out);
    return DMSA_OK;
}

// decided here, self-describing (include/dmsa_dense_normals.h, N5): width = n, height = 1, the identity viewpoint, the counts twelve digits wide
int dmsa_pcd_header_normals_binary(int64_t n, char* out, int32_t cap) {
    if (n < 0 || n >= 1000000000000ll || !out || cap < 1) return DMSA_ERR_INVALID;
    const int len = std::snprintf(out, (size_t)cap,
                                  "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z normal_x normal_y normal_z curvature\nSIZE 4 4 4 4 4 4 4\n"
                                  "TYPE F F F F F F F\nCOUNT 1 1 1 1 1 1 1\nWIDTH %012lld\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %012lld\nDATA binary\n",
                                  (long long)n, (long long)n);
    if (len < 0 || len >= cap) return DMSA_ERR_INVALID;
    return len;
}

}  // extern "C"
