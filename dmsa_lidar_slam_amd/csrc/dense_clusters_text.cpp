// dense_clusters_text.cpp — the host-only side of include/dmsa_dense_clusters.h: the defaults, what C1 asks of the two sizes, and the header
// of C7.  No device, no context.
#include "../../include/dmsa_dense_clusters.h"

#include <cstdio>

const char* dense_cluster_config_refusal(const dmsa_dense_cluster_config* cfg);

// C1, the sizes alone: the reason of the first breach, or nullptr
const char* dense_cluster_config_refusal(const dmsa_dense_cluster_config* cfg) {
    constexpr int32_t kMax = 1 << 26;
    if (cfg->min_size < 1 || cfg->min_size > kMax) return "min_size must lie in [1, 2^26]";
    if (cfg->max_size != 0 && (cfg->max_size < cfg->min_size || cfg->max_size > kMax)) return "max_size must be 0 or lie in [min_size, 2^26]";
    return nullptr;
}

extern "C" {

// min_size comes from no recorded data: a placeholder for a caller who names none
void dmsa_default_dense_cluster_config(dmsa_dense_cluster_config* cfg) {
    if (!cfg) return;
    cfg->radius = 0.3f, cfg->min_size = 50, cfg->max_size = 0, cfg->pad = 0;
}

// decided here (C7): the x y z header with an unsigned 4-byte label as its last field; width = n, height = 1, the identity viewpoint, the
// counts twelve digits wide
int dmsa_pcd_header_xyz_label_binary(int64_t n, int32_t intensity, char* out, int32_t cap) {
    if (n < 0 || n >= 1000000000000ll || !out || cap < 1) return DMSA_ERR_INVALID;
    const int len = std::snprintf(out, (size_t)cap,
                                  "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z %slabel\nSIZE 4 4 4 %s4\nTYPE F F F %sU\nCOUNT 1 1 1 %s1\n"
                                  "WIDTH %012lld\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %012lld\nDATA binary\n",
                                  intensity ? "intensity " : "", intensity ? "4 " : "", intensity ? "F " : "", intensity ? "1 " : "", (long long)n, (long long)n);
    if (len < 0 || len >= cap) return DMSA_ERR_INVALID;
    return len;
}

}  // extern "C"
