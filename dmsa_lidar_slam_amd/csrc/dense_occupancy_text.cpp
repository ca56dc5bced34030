// dense_occupancy_text.cpp — the host-only side of include/dmsa_dense_occupancy.h: the defaults, M1's checks of the config alone, M5 on the
// host through the header the device kernels compile (dense_occupancy_rule.h), and the texts of M6 and M7: the PCD header, the PGM header and
// the YAML.  No device, no context.  Built with -ffp-contract=off.
#include "../../include/dmsa_dense_occupancy.h"

#include "dense_occupancy_rule.h"

#include <cmath>
#include <cstdio>
#include <cstring>

using namespace dmsa;

const char* dense_occupancy_rule_refusal(const dmsa_dense_occupancy_config* cfg);
const char* dense_occupancy_config_refusal(const dmsa_dense_occupancy_config* cfg);

namespace {
constexpr int32_t kMaxThreshold = 1 << 20;
bool threshold(const int32_t v) { return v >= 1 && v <= kMaxThreshold; }
}  // namespace

// M1, the four integers of M5: the reason of the first breach, or nullptr
const char* dense_occupancy_rule_refusal(const dmsa_dense_occupancy_config* cfg) {
    if (!threshold(cfg->min_hits)) return "min_hits must lie in [1, 2^20]";
    if (!threshold(cfg->min_passes)) return "min_passes must lie in [1, 2^20]";
    if (!threshold(cfg->occ_num)) return "occ_num must lie in [1, 2^20]";
    if (!threshold(cfg->occ_den)) return "occ_den must lie in [1, 2^20]";
    return nullptr;
}
// M1, the config alone, cell_size apart (that one is measured against the voxel)
const char* dense_occupancy_config_refusal(const dmsa_dense_occupancy_config* cfg) {
    if (!std::isfinite(cfg->max_length)) return "max_length must be finite";
    if (!(cfg->max_length > 0.0f)) return "max_length must be > 0";
    if (const char* why = dense_occupancy_rule_refusal(cfg)) return why;
    const int64_t s = cfg->initial_slots;
    if (s != 0 && (s < 64 || s > ((int64_t)1 << 31) || (s & (s - 1)) != 0)) return "initial_slots must be 0 or a power of two in [64, 2^31]";
    return nullptr;
}

extern "C" {

void dmsa_default_dense_occupancy_config(dmsa_dense_occupancy_config* cfg) {
    if (!cfg) return;
    // from the toy scene of DESIGN.md section 9, not from recorded data
    cfg->cell_size = 0.2f, cfg->max_length = 30.0f;
    cfg->min_hits = 1, cfg->min_passes = 2, cfg->occ_num = 16, cfg->occ_den = 1;
    cfg->initial_slots = 0;
}

int dmsa_dense_occupancy_state(const dmsa_dense_occupancy_config* cfg, uint32_t hits, uint32_t passes) {
    if (!cfg || dense_occupancy_rule_refusal(cfg)) return DMSA_ERR_INVALID;
    return (int)occupancy_state((uint32_t)cfg->min_hits, (uint32_t)cfg->min_passes, (uint32_t)cfg->occ_num, (uint32_t)cfg->occ_den, hits, passes);
}

// decided here (M6): three floats and three unsigned 4-byte fields; width = n, height = 1, the identity viewpoint, the counts twelve digits wide
int dmsa_pcd_header_occupancy_binary(int64_t n, char* out, int32_t cap) {
    if (n < 0 || n >= 1000000000000ll || !out || cap < 1) return DMSA_ERR_INVALID;
    const int len = std::snprintf(out, (size_t)cap,
                                  "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z hits passes state\nSIZE 4 4 4 4 4 4\nTYPE F F F U U U\n"
                                  "COUNT 1 1 1 1 1 1\nWIDTH %012lld\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %012lld\nDATA binary\n",
                                  (long long)n, (long long)n);
    if (len < 0 || len >= cap) return DMSA_ERR_INVALID;
    return len;
}

int dmsa_occupancy_map_pgm_header(int32_t width, int32_t height, char* out, int32_t cap) {
    if (width < 1 || height < 1 || !out || cap < 1) return DMSA_ERR_INVALID;
    const int len = std::snprintf(out, (size_t)cap, "P5\n%d %d\n255\n", (int)width, (int)height);
    if (len < 0 || len >= cap) return DMSA_ERR_INVALID;
    return len;
}

int dmsa_occupancy_map_yaml(const char* pgm_path, float cell_size, int32_t cx_min, int32_t cy_min, char* out, int32_t cap) {
    if (!pgm_path || !out || cap < 1 || !std::isfinite(cell_size) || !(cell_size > 0.0f)) return DMSA_ERR_INVALID;
    const char* slash = std::strrchr(pgm_path, '/');
    const char* name = slash ? slash + 1 : pgm_path;
    const double c = (double)cell_size;
    const int len = std::snprintf(out, (size_t)cap, "image: %s\nresolution: %.9g\norigin: [%.9g, %.9g, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n", name, c,
                                  (double)cx_min * c, (double)cy_min * c);
    if (len < 0 || len >= cap) return DMSA_ERR_INVALID;
    return len;
}

}  // extern "C"
