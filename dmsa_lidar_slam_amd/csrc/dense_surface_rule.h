// dense_surface_rule.h — the arithmetic of include/dmsa_dense_surface.h for ONE ray (S3-S4), ONE cell (S7) and ONE tetrahedron (S8), stated once
// for the device kernels (csrc/dense_surface.hip) and for the host-only call dmsa_dense_surface_samples (csrc/dense_surface_text.cpp), as
// dense_carve_walk.h is for T2-T5 and dense_occupancy_rule.h for M5.  Every translation unit that includes it is built with
// -ffp-contract=off: each float and double operation below is rounded on its own.
#pragma once
#include <cmath>
#include <cstdint>

#include "dense_occupancy_rule.h"

namespace dmsa {

constexpr int32_t kSurfaceMaxWeight = 1 << 20;  // S1: min_weight
constexpr float kSurfaceScale = 32768.0f;       // S4: q = 2^15 at +truncation

// S3: the ends a -> b of the segment a ray integrates
struct SurfaceSegment {
    float ax, ay, az, bx, by, bz;
};
DMSA_CARVE_HD SurfaceSegment surface_segment(const CarveRay& r, const float ox, const float oy, const float oz, const float gx, const float gy, const float gz,
                                             const float truncation) {
    const float f = carve_div(truncation, r.L);
    const float px = f * r.dx, py = f * r.dy, pz = f * r.dz;
    SurfaceSegment s;
    s.bx = gx + px, s.by = gy + py, s.bz = gz + pz;
    const bool behind = r.L > truncation;  // the segment starts one truncation in front of the endpoint, or at the origin if that is nearer
    s.ax = behind ? gx - px : ox, s.ay = behind ? gy - py : oy, s.az = behind ? gz - pz : oz;
    return s;
}

// S4: the sample of the ray (r, ending at g) in cell (cx, cy, cz)
DMSA_CARVE_HD int32_t surface_sample(const CarveRay& r, const float gx, const float gy, const float gz, const int32_t cx, const int32_t cy, const int32_t cz,
                                     const double cell, const float truncation) {
    const float ux = gx - occupancy_centre(cx, cell), uy = gy - occupancy_centre(cy, cell), uz = gz - occupancy_centre(cz, cell);
    float s = ux * r.dx;
    s += uy * r.dy;
    s += uz * r.dz;
    s = carve_div(s, r.L);
    s = fminf(fmaxf(s, -truncation), truncation);
    return (int32_t)rintf(carve_div(s, truncation) * kSurfaceScale);
}

// S7: the field of a cell in metres
DMSA_CARVE_HD float surface_tsdf(const int64_t sum, const uint32_t n, const float truncation) {
    return (float)((((double)sum / (double)n) / 32768.0) * (double)truncation);
}

// S8: where the field crosses zero between the lower node (cell c0 on this axis, sums sum0 / n0) and the upper one, `off` (0 or 1) cells further
DMSA_CARVE_HD double surface_crossing(const int64_t sum0, const uint32_t n0, const int64_t sum1, const uint32_t n1) {
    const double m0 = (double)sum0 / (double)n0, m1 = (double)sum1 / (double)n1;
    return m0 / (m0 - m1);
}
DMSA_CARVE_HD float surface_vertex_axis(const int32_t c0, const double t, const int32_t off, const double cell) {
    return (float)((((double)c0 + 0.5) + t * (double)off) * cell);
}

// S8: the corner masks v0..v3 of Kuhn tetrahedron t (0..5: the permutations xyz, xzy, yxz, yzx, zxy, zyx), one per byte, v0 lowest
DMSA_CARVE_HD uint32_t surface_chain(const int t) {
    const int a = t >> 1, b = (t & 1) ? (a == 2 ? 1 : 2) : (a == 0 ? 1 : 0);
    const uint32_t v1 = 1u << a, v2 = v1 | (1u << b);
    return (v1 << 8) | (v2 << 16) | (7u << 24);
}
DMSA_CARVE_HD uint32_t surface_chain_mask(const uint32_t chain, const int position) { return (chain >> (8 * position)) & 7u; }

// an edge of the chain as four bits: the lower position << 2 | the upper one
DMSA_CARVE_HD uint32_t surface_edge(const int i, const int j) { return i < j ? (uint32_t)(i << 2 | j) : (uint32_t)(j << 2 | i); }
DMSA_CARVE_HD int surface_low_bit(const uint32_t four) { return (four & 1u) ? 0 : (four & 2u) ? 1 : (four & 4u) ? 2 : 3; }
DMSA_CARVE_HD int surface_high_bit(const uint32_t four) { return (four & 8u) ? 3 : (four & 4u) ? 2 : (four & 2u) ? 1 : 0; }

// S8: the triangles of a tetrahedron whose four nodes are valid, from the set `in4` of its chain positions that are inside: the count in bits
// 24.., triangle k in bits 12 k .. 12 k + 11, its three corners four bits each (surface_edge), first corner lowest.  Before orientation.
DMSA_CARVE_HD uint32_t surface_tetra_triangles(const uint32_t in4) {
    const uint32_t out4 = ~in4 & 15u;
    const int k = (int)((in4 & 1u) + (in4 >> 1 & 1u) + (in4 >> 2 & 1u) + (in4 >> 3 & 1u));
    if (k == 0 || k == 4) return 0u;
    if (k == 2) {
        const int A = surface_low_bit(in4), B = surface_high_bit(in4), Cc = surface_low_bit(out4), D = surface_high_bit(out4);
        const uint32_t ac = surface_edge(A, Cc), ad = surface_edge(A, D), bd = surface_edge(B, D), bc = surface_edge(B, Cc);
        return (2u << 24) | ((ac | bd << 4 | bc << 8) << 12) | (ac | ad << 4 | bd << 8);
    }
    const int A = surface_low_bit(k == 1 ? in4 : out4);  // the corner that is alone on its side
    uint32_t tri = 0u;
    int at = 0;
    for (int x = 0; x < 4; ++x)
        if (x != A) tri |= surface_edge(A, x) << (4 * at++);
    return (1u << 24) | tri;
}

// S8, ORIENTATION, derived once per call on the host in integers: bit 2 * in4 + k of flip[t] says that triangle k of tetrahedron t with the
// inside set in4 has its last two corners swapped.  Doubled lattice coordinates, so that the crossings at the edge midpoints are integers:
// N = (v1 - v0) x (v2 - v0) dotted with (centroid of the outside corners - centroid of the inside ones), scaled by both counts, is made
// positive.
struct SurfaceOrientation {
    uint32_t flip[6];
};
inline SurfaceOrientation surface_orientation() {
    SurfaceOrientation o{};
    for (int t = 0; t < 6; ++t) {
        const uint32_t chain = surface_chain(t);
        int corner[4][3];
        for (int p = 0; p < 4; ++p)
            for (int a = 0; a < 3; ++a) corner[p][a] = (int)(surface_chain_mask(chain, p) >> a & 1u);
        for (uint32_t in4 = 1; in4 < 15; ++in4) {
            int n_in = 0, n_out = 0, s_in[3] = {0, 0, 0}, s_out[3] = {0, 0, 0};
            for (int p = 0; p < 4; ++p)
                for (int a = 0; a < 3; ++a) (in4 >> p & 1u) ? (s_in[a] += 2 * corner[p][a]) : (s_out[a] += 2 * corner[p][a]);
            for (int p = 0; p < 4; ++p) (in4 >> p & 1u) ? ++n_in : ++n_out;
            const uint32_t tris = surface_tetra_triangles(in4);
            for (uint32_t k = 0; k < (tris >> 24); ++k) {
                int v[3][3];
                for (int c = 0; c < 3; ++c) {
                    const uint32_t e = (tris >> (12 * k + 4 * c)) & 15u;
                    for (int a = 0; a < 3; ++a) v[c][a] = corner[e >> 2][a] + corner[e & 3u][a];
                }
                const int e1[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]}, e2[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
                const int nrm[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
                int dot = 0;
                for (int a = 0; a < 3; ++a) dot += nrm[a] * (n_in * s_out[a] - n_out * s_in[a]);
                if (dot < 0) o.flip[t] |= 1u << (2 * in4 + k);
            }
        }
    }
    return o;
}

}  // namespace dmsa
