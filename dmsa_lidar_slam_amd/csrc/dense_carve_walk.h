// dense_carve_walk.h — T2-T5 of include/dmsa_dense_carve.h for ONE ray, stated once for the device kernels (csrc/dense_carve.hip) and for the
// host-only calls dmsa_dense_carve_walk / dmsa_dense_carve_sees_through (csrc/dense_carve_text.cpp), as pcl_eigen33.h is for N4: the ray's
// length, the fixed-point ends, the integer walk from cell to cell, the hash of a walk and the float pair test.  Every translation unit that
// includes it is built with -ffp-contract=off: each float operation below is rounded on its own.  The walk's state is nine 32-bit and six
// 64-bit integers touched by name only, so a kernel keeps it in registers.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define DMSA_CARVE_HD __host__ __device__ __forceinline__
#else
#define DMSA_CARVE_HD inline
#endif

namespace dmsa {

constexpr int64_t kCarveUnit = 1024;          // T3: 2^S
constexpr int64_t kCarveW = 2 * kCarveUnit;   // cell planes in X units
constexpr int32_t kCarveMaxExtent = 1 << 11;  // T2: end cells further apart on an axis skip the ray
constexpr int32_t kCarveMaxSteps = 3 * kCarveMaxExtent;
constexpr int32_t kCarveCellBias = 1 << 20;   // rows live in cells [-2^20, 2^20)

// sqrtf and `/` are correctly rounded on the host and, with hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt, on the device (the
// __fsqrt_rn of the HIP headers is the hardware's approximate square root unless OCML_BASIC_ROUNDED_OPERATIONS is defined: not used here)
DMSA_CARVE_HD float carve_sqrt(const float x) { return sqrtf(x); }
DMSA_CARVE_HD float carve_div(const float a, const float b) { return a / b; }

// T2: d = g - o and its length
struct CarveRay {
    float dx, dy, dz, L2, L;
};
DMSA_CARVE_HD CarveRay carve_ray(const float ox, const float oy, const float oz, const float gx, const float gy, const float gz) {
    CarveRay r;
    r.dx = gx - ox, r.dy = gy - oy, r.dz = gz - oz;
    float l2 = r.dx * r.dx;
    l2 += r.dy * r.dy;
    l2 += r.dz * r.dz;
    r.L2 = l2, r.L = carve_sqrt(l2);
    return r;
}
// T2's first two cases
DMSA_CARVE_HD bool carve_ray_skipped(const CarveRay& r, const float max_length) { return r.L2 == 0.0f || r.L > max_length; }

// T4: the cell the walk stands in and what it needs to find the next one
struct CarveWalk {
    int64_t nx, ny, nz;  // distance in X units from A to the next plane, per axis
    int64_t dx, dy, dz;  // |B - A|
    int32_t cx, cy, cz;  // the cell
    int32_t lx, ly, lz;  // planes left to cross
    int32_t sx, sy, sz;  // direction of travel: -1, 0, 1
};

// T3 and T4's set-up for one axis; false: T2's third case
DMSA_CARVE_HD bool carve_axis(const float a, const float b, const double c, int64_t* n, int64_t* d, int32_t* cell, int32_t* left, int32_t* sign) {
    const double pa = (double)a / c, pb = (double)b / c;
    if (!(fabs(pa) < 2147483648.0) || !(fabs(pb) < 2147483648.0)) return false;
    const int64_t fa = (int64_t)floor(pa * 1024.0), fb = (int64_t)floor(pb * 1024.0);
    const int64_t xa = 2 * fa + 1, xb = 2 * fb + 1;
    const int64_t ca = fa >> 10, cb = fb >> 10;  // (arithmetic shifts: floor)
    const int64_t diff = xb - xa, cells = cb - ca;
    const int64_t l = cells < 0 ? -cells : cells;
    if (l > (int64_t)kCarveMaxExtent) return false;
    *d = diff < 0 ? -diff : diff;
    *sign = diff > 0 ? 1 : (diff < 0 ? -1 : 0);
    *cell = (int32_t)ca, *left = (int32_t)l;
    const int64_t in_cell = xa & (kCarveW - 1);  // xa - W * ca: odd, 1 .. W - 1
    *n = diff > 0 ? kCarveW - in_cell : in_cell;
    return true;
}
// the walk placed in the origin's cell; false: the ray is skipped (T2's third case)
DMSA_CARVE_HD bool carve_walk_begin(const double c, const float ox, const float oy, const float oz, const float gx, const float gy, const float gz, CarveWalk* w) {
    const bool x = carve_axis(ox, gx, c, &w->nx, &w->dx, &w->cx, &w->lx, &w->sx);
    const bool y = carve_axis(oy, gy, c, &w->ny, &w->dy, &w->cy, &w->ly, &w->sy);
    const bool z = carve_axis(oz, gz, c, &w->nz, &w->dz, &w->cz, &w->lz, &w->sz);
    return x && y && z;
}
// to the next traversed cell; false: the walk stood in the endpoint's cell already
DMSA_CARVE_HD bool carve_walk_step(CarveWalk* w) {
    const bool ax = w->lx > 0, ay = w->ly > 0, az = w->lz > 0;
    if (!(ax || ay || az)) return false;
    // n_a / d_a against n_b / d_b by cross-multiplication: below 2^47 each
    const int64_t xy = w->nx * w->dy, yx = w->ny * w->dx;
    const int64_t xz = w->nx * w->dz, zx = w->nz * w->dx;
    const int64_t yz = w->ny * w->dz, zy = w->nz * w->dy;
    const bool tx = ax && (!ay || xy <= yx) && (!az || xz <= zx);
    const bool ty = ay && (!ax || yx <= xy) && (!az || yz <= zy);
    const bool tz = az && (!ax || zx <= xz) && (!ay || zy <= yz);
    if (tx) w->cx += w->sx, w->nx += kCarveW, w->lx -= 1;
    if (ty) w->cy += w->sy, w->ny += kCarveW, w->ly -= 1;
    if (tz) w->cz += w->sz, w->nz += kCarveW, w->lz -= 1;
    return true;
}
DMSA_CARVE_HD bool carve_cell_holds_rows(const CarveWalk& w) {
    return w.cx >= -kCarveCellBias && w.cx < kCarveCellBias && w.cy >= -kCarveCellBias && w.cy < kCarveCellBias && w.cz >= -kCarveCellBias && w.cz < kCarveCellBias;
}

// THE HASH of the header
constexpr unsigned long long kCarveHashSeed = 0xCBF29CE484222325ull, kCarveHashMul = 0x100000001B3ull;
DMSA_CARVE_HD unsigned long long carve_hash_cell(unsigned long long h, const CarveWalk& w) {
    h = (h ^ (unsigned long long)((long long)w.cx + kCarveCellBias)) * kCarveHashMul;
    h = (h ^ (unsigned long long)((long long)w.cy + kCarveCellBias)) * kCarveHashMul;
    h = (h ^ (unsigned long long)((long long)w.cz + kCarveCellBias)) * kCarveHashMul;
    return h;
}

// T5's constants, computed once per call
struct CarvePair {
    float rho2, tan_half_angle, end_margin, start_margin;
};
DMSA_CARVE_HD CarvePair carve_pair(const float rho, const float tan_half_angle, const float end_margin, const float start_margin) {
    return CarvePair{rho * rho, tan_half_angle, end_margin, start_margin};
}
// T5: does the ray (r, ending at g) see through the point p
DMSA_CARVE_HD bool carve_sees_through(const CarveRay& r, const CarvePair& k, const float gx, const float gy, const float gz, const float px, const float py,
                                      const float pz) {
    const float ux = gx - px, uy = gy - py, uz = gz - pz;
    float rem = ux * r.dx;
    rem += uy * r.dy;
    rem += uz * r.dz;
    rem = carve_div(rem, r.L);
    float u2 = ux * ux;
    u2 += uy * uy;
    u2 += uz * uz;
    const float perp2 = u2 - rem * rem;
    const float s = r.L - rem;
    const float w = k.tan_half_angle * rem;
    return s >= k.start_margin && rem >= k.end_margin && perp2 <= k.rho2 && perp2 <= w * w;
}

}  // namespace dmsa
