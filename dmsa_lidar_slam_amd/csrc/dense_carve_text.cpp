// dense_carve_text.cpp — the host-only side of include/dmsa_dense_carve.h: the defaults, T1's checks of the config alone, and the walk and the
// pair test of ONE ray through the header the device kernels compile (dense_carve_walk.h).  No device, no context.  Built with
// -ffp-contract=off: every operation of T2 and T5 is rounded on its own.
#include "../../include/dmsa_dense_carve.h"

#include "dense_carve_walk.h"

#include <cmath>

using namespace dmsa;

const char* dense_carve_config_refusal(const dmsa_dense_carve_config* cfg) {
    if (!std::isfinite(cfg->rho) || !std::isfinite(cfg->end_margin) || !std::isfinite(cfg->start_margin) || !std::isfinite(cfg->max_length))
        return "rho, end_margin, start_margin and max_length must be finite";
    if (!(cfg->rho > 0.0f)) return "rho must be > 0";
    if (!(cfg->end_margin > 0.0f)) return "end_margin must be > 0";
    if (!(cfg->start_margin >= 0.0f)) return "start_margin must be >= 0";
    if (!(cfg->max_length > 0.0f)) return "max_length must be > 0";
    if (!(cfg->tan_half_angle > 0.0f && cfg->tan_half_angle <= 1.0f)) return "tan_half_angle must lie in (0, 1]";
    if (cfg->min_passes < 1 || cfg->min_passes > (1 << 20)) return "min_passes must lie in [1, 2^20]";
    return nullptr;
}

extern "C" {

void dmsa_default_dense_carve_config(dmsa_dense_carve_config* cfg) {
    if (!cfg) return;
    // from the toy scene of DESIGN.md section 9, not from recorded data
    cfg->cell_size = 0.2f, cfg->rho = 0.1f, cfg->tan_half_angle = 0.052407779f, cfg->end_margin = 0.3f, cfg->start_margin = 0.5f, cfg->max_length = 30.0f;
    cfg->min_passes = 2, cfg->pad = 0;
}

int dmsa_dense_carve_walk(float cell_size, const float* o, const float* g, int32_t* cells_xyz, int64_t cap, int64_t* n) {
    if (n) *n = 0;
    if (!o || !g || !n || cap < 0 || (cap > 0 && !cells_xyz) || !std::isfinite(cell_size) || !(cell_size > 0.0f)) return DMSA_ERR_INVALID;
    const CarveRay ray = carve_ray(o[0], o[1], o[2], g[0], g[1], g[2]);
    CarveWalk w;
    if (ray.L2 == 0.0f || !carve_walk_begin((double)cell_size, o[0], o[1], o[2], g[0], g[1], g[2], &w)) {
        *n = -1;
        return DMSA_OK;
    }
    int64_t cells = 0;
    for (int32_t step = 0; step <= kCarveMaxSteps; ++step) {
        if (cells < cap) cells_xyz[3 * cells] = w.cx, cells_xyz[3 * cells + 1] = w.cy, cells_xyz[3 * cells + 2] = w.cz;
        ++cells;
        if (!carve_walk_step(&w)) break;
    }
    *n = cells;
    return DMSA_OK;
}

int dmsa_dense_carve_sees_through(const dmsa_dense_carve_config* cfg, const float* o, const float* g, const float* p) {
    if (!cfg || !o || !g || !p || dense_carve_config_refusal(cfg)) return DMSA_ERR_INVALID;
    const CarveRay ray = carve_ray(o[0], o[1], o[2], g[0], g[1], g[2]);
    if (carve_ray_skipped(ray, cfg->max_length)) return 0;
    return carve_sees_through(ray, carve_pair(cfg->rho, cfg->tan_half_angle, cfg->end_margin, cfg->start_margin), g[0], g[1], g[2], p[0], p[1], p[2]) ? 1 : 0;
}

}  // extern "C"
