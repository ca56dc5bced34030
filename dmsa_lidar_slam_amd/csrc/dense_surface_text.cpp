// dense_surface_text.cpp — the host-only side of include/dmsa_dense_surface.h: the defaults, S1's checks of the config alone, S2-S4 for one
// ray on the host through the header the device kernels compile (dense_surface_rule.h), and the texts of S7 and S9: the PCD header and the
// PLY header.  No device, no context.  Built with -ffp-contract=off.
#include "../../include/dmsa_dense_surface.h"

#include "dense_surface_rule.h"

#include <cmath>
#include <cstdio>

using namespace dmsa;

const char* dense_surface_weight_refusal(int32_t min_weight);
const char* dense_surface_config_refusal(const dmsa_dense_surface_config* cfg);

const char* dense_surface_weight_refusal(int32_t min_weight) {
    return min_weight >= 1 && min_weight <= kSurfaceMaxWeight ? nullptr : "min_weight must lie in [1, 2^20]";
}
// S1, the config alone, cell_size against the voxel apart (that needs the store): the reason of the first breach, or nullptr
const char* dense_surface_config_refusal(const dmsa_dense_surface_config* cfg) {
    if (!std::isfinite(cfg->truncation)) return "truncation must be finite";
    if (!(cfg->truncation >= cfg->cell_size) || !(cfg->truncation <= 16.0f * cfg->cell_size)) return "truncation must lie in [cell_size, 16 * cell_size]";
    if (!std::isfinite(cfg->max_length)) return "max_length must be finite";
    if (!(cfg->max_length > 0.0f)) return "max_length must be > 0";
    if (const char* why = dense_surface_weight_refusal(cfg->min_weight)) return why;
    const int64_t s = cfg->initial_slots;
    if (s != 0 && (s < 64 || s > ((int64_t)1 << 31) || (s & (s - 1)) != 0)) return "initial_slots must be 0 or a power of two in [64, 2^31]";
    return nullptr;
}

extern "C" {

void dmsa_default_dense_surface_config(dmsa_dense_surface_config* cfg) {
    if (!cfg) return;
    // placeholders from the toy scene of DESIGN.md section 9, not from recorded data
    cfg->cell_size = 0.2f, cfg->truncation = 0.6f, cfg->max_length = 30.0f;
    cfg->min_weight = 2, cfg->initial_slots = 0;
}

int dmsa_dense_surface_samples(const dmsa_dense_surface_config* cfg, const float* o, const float* g, int32_t* cells_xyz, int32_t* q, int64_t cap, int64_t* n) {
    if (n) *n = 0;
    if (!cfg || !o || !g || !n || cap < 0 || (cap > 0 && (!cells_xyz || !q))) return DMSA_ERR_INVALID;
    if (!std::isfinite(cfg->cell_size) || !(cfg->cell_size > 0.0f) || dense_surface_config_refusal(cfg)) return DMSA_ERR_INVALID;
    const double c = (double)cfg->cell_size;
    const CarveRay ray = carve_ray(o[0], o[1], o[2], g[0], g[1], g[2]);
    CarveWalk w;
    *n = -1;
    if (carve_ray_skipped(ray, cfg->max_length)) return DMSA_OK;
    const SurfaceSegment s = surface_segment(ray, o[0], o[1], o[2], g[0], g[1], g[2], cfg->truncation);
    if (!carve_walk_begin(c, s.ax, s.ay, s.az, s.bx, s.by, s.bz, &w)) return DMSA_OK;
    int64_t samples = 0;
    for (int32_t step = 0; step <= kCarveMaxSteps; ++step) {
        if (carve_cell_holds_rows(w)) {
            if (samples < cap) {
                cells_xyz[3 * samples] = w.cx, cells_xyz[3 * samples + 1] = w.cy, cells_xyz[3 * samples + 2] = w.cz;
                q[samples] = surface_sample(ray, g[0], g[1], g[2], w.cx, w.cy, w.cz, c, cfg->truncation);
            }
            ++samples;
        }
        if (!carve_walk_step(&w)) break;
    }
    *n = samples;
    return DMSA_OK;
}

// decided here (S7): four floats and one unsigned 4-byte field; width = n, height = 1, the identity viewpoint, the counts twelve digits wide
int dmsa_pcd_header_tsdf_binary(int64_t n, char* out, int32_t cap) {
    if (n < 0 || n >= 1000000000000ll || !out || cap < 1) return DMSA_ERR_INVALID;
    const int len = std::snprintf(out, (size_t)cap,
                                  "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z tsdf weight\nSIZE 4 4 4 4 4\nTYPE F F F F U\n"
                                  "COUNT 1 1 1 1 1\nWIDTH %012lld\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %012lld\nDATA binary\n",
                                  (long long)n, (long long)n);
    if (len < 0 || len >= cap) return DMSA_ERR_INVALID;
    return len;
}

int dmsa_ply_header_mesh(int64_t vertices, int64_t triangles, char* out, int32_t cap) {
    if (vertices < 0 || vertices > 2147483647ll || triangles < 0 || triangles > 2147483647ll || !out || cap < 1) return DMSA_ERR_INVALID;
    const int len = std::snprintf(out, (size_t)cap,
                                  "ply\nformat binary_little_endian 1.0\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\n"
                                  "element face %lld\nproperty list uchar int vertex_indices\nend_header\n",
                                  (long long)vertices, (long long)triangles);
    if (len < 0 || len >= cap) return DMSA_ERR_INVALID;
    return len;
}

}  // extern "C"
