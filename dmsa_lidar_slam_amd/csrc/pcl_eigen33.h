// pcl_eigen33.h — pcl::computeRoots2 / computeRoots / eigen33 (pcl/common/impl/eigen.hpp, PCL 1.10: smallest eigenvalue and its vector, float),
// the curvature of pcl::solvePlaneParameters and pcl::flipNormalTowardsViewpoint, stated once for the two places that turn a 3 x 3 float
// covariance into a normal: k_knn_normals (static_kernels.hip, the keyframe clouds) and the dense cloud's normals (dense_normals.hip on the
// device, dmsa_dense_normal_from_moments on the host).  atan2 / cos / sin come from include/dmsa_detmath.h: fixed sequences of correctly
// rounded IEEE operations, so host and device return the same bits.  Everything else is +, -, *, /, sqrtf, each rounded on its own: build
// with -ffp-contract=off.  Compiles as plain C++ (host-only translation units) and as HIP.
#pragma once
#include <cfloat>
#include <cmath>

#include "../../include/dmsa_detmath.h"

#if defined(__HIPCC__)
#define DMSA_PCL_HD __host__ __device__ __forceinline__
#else
#define DMSA_PCL_HD inline
#endif

namespace dmsa {

DMSA_PCL_HD void pcl_roots2(float b, float c, float* roots) {
    roots[0] = 0.0f;
    float d = (float)((double)(b * b) - 4.0 * (double)c);  // Scalar (b * b - 4.0 * c): the subtraction runs in double
    if (d < 0.0f) d = 0.0f;
    const float sd = sqrtf(d);
    roots[2] = 0.5f * (b + sd);
    roots[1] = 0.5f * (b - sd);
}
DMSA_PCL_HD void pcl_roots(const float* m /* row-major 3x3 */, float* roots) {
    const float m00 = m[0], m01 = m[1], m02 = m[2], m11 = m[4], m12 = m[5], m22 = m[8];
    const float c0 = m00 * m11 * m22 + 2.0f * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01;
    const float c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12;
    const float c2 = m00 + m11 + m22;
    if (fabsf(c0) < FLT_EPSILON) {
        pcl_roots2(c2, c1, roots);
        return;
    }
    const float s_inv3 = (float)(1.0 / 3.0), s_sqrt3 = sqrtf(3.0f);
    const float c2_over_3 = c2 * s_inv3;
    float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
    if (a_over_3 > 0.0f) a_over_3 = 0.0f;
    const float half_b = 0.5f * (c0 + c2_over_3 * (2.0f * c2_over_3 * c2_over_3 - c1));
    float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
    if (q > 0.0f) q = 0.0f;
    const float rho = sqrtf(-a_over_3);
    // float atan2 / cos / sin as a correctly rounded libm returns them: evaluated in double, rounded once (glibc's sinf / cosf work
    // the same way; device and host double functions agree after the rounding, so normals are reproducible across the two)
    const float theta = (float)dmsa_det::det_atan2((double)sqrtf(-q), (double)half_b) * s_inv3;
    const float cos_theta = (float)dmsa_det::det_cos((double)theta), sin_theta = (float)dmsa_det::det_sin((double)theta);
    roots[0] = c2_over_3 + 2.0f * rho * cos_theta;
    roots[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
    roots[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
    float t;
    if (roots[0] >= roots[1]) t = roots[0], roots[0] = roots[1], roots[1] = t;
    if (roots[1] >= roots[2]) {
        t = roots[1], roots[1] = roots[2], roots[2] = t;
        if (roots[0] >= roots[1]) t = roots[0], roots[0] = roots[1], roots[1] = t;
    }
    if (roots[0] <= 0.0f) pcl_roots2(c2, c1, roots);
}

// pcl::solvePlaneParameters -> pcl::eigen33 (smallest eigenvalue) on the full symmetric cov[9], the curvature |lambda_0 / trace|, and
// pcl::flipNormalTowardsViewpoint with the view vector w = viewpoint - point: out = (nx, ny, nz, curvature)
DMSA_PCL_HD void pcl_plane_normal(const float* cov /* row-major 3x3 */, const float wx, const float wy, const float wz, float* out) {
    float scale = 0.0f;
#pragma unroll
    for (int e = 0; e < 9; ++e) scale = fmaxf(scale, fabsf(cov[e]));
    if (scale <= FLT_MIN) scale = 1.0f;
    float sm[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) sm[e] = cov[e] / scale;
    float roots[3];
    pcl_roots(sm, roots);
    const float eigenvalue = roots[0] * scale;
    sm[0] -= roots[0], sm[4] -= roots[0], sm[8] -= roots[0];
    const float r0x = sm[0], r0y = sm[1], r0z = sm[2], r1x = sm[3], r1y = sm[4], r1z = sm[5], r2x = sm[6], r2y = sm[7], r2z = sm[8];
    const float v1x = r0y * r1z - r0z * r1y, v1y = r0z * r1x - r0x * r1z, v1z = r0x * r1y - r0y * r1x;
    const float v2x = r0y * r2z - r0z * r2y, v2y = r0z * r2x - r0x * r2z, v2z = r0x * r2y - r0y * r2x;
    const float v3x = r1y * r2z - r1z * r2y, v3y = r1z * r2x - r1x * r2z, v3z = r1x * r2y - r1y * r2x;
    const float len1 = v1x * v1x + (v1y * v1y + v1z * v1z), len2 = v2x * v2x + (v2y * v2y + v2z * v2z), len3 = v3x * v3x + (v3y * v3y + v3z * v3z);
    float nx, ny, nz;
    if (len1 >= len2 && len1 >= len3) {
        const float s = sqrtf(len1);
        nx = v1x / s, ny = v1y / s, nz = v1z / s;
    } else if (len2 >= len1 && len2 >= len3) {
        const float s = sqrtf(len2);
        nx = v2x / s, ny = v2y / s, nz = v2z / s;
    } else {
        const float s = sqrtf(len3);
        nx = v3x / s, ny = v3y / s, nz = v3z / s;
    }
    const float eig_sum = cov[0] + cov[4] + cov[8];
    const float curvature = eig_sum != 0.0f ? fabsf(eigenvalue / eig_sum) : 0.0f;
    // pcl::flipNormalTowardsViewpoint
    const float cos_theta = wx * nx + wy * ny + wz * nz;
    if (cos_theta < 0.0f) nx *= -1.0f, ny *= -1.0f, nz *= -1.0f;
    out[0] = nx, out[1] = ny, out[2] = nz, out[3] = curvature;
}

// N4 of include/dmsa_dense_normals.h: the ten integer moments (n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz) of a neighbourhood -> the normal.
// Fewer than max(3, min_neighbours) neighbours: four quiet NaNs (false is returned).
DMSA_PCL_HD bool dense_normal_from_moments(const long long* m, const float wx, const float wy, const float wz, const int min_neighbours, float* out) {
    const long long need = min_neighbours > 3 ? min_neighbours : 3;
    if (m[0] < need) {
        union { unsigned u; float f; } nanv;
        nanv.u = 0x7fc00000u;
        out[0] = out[1] = out[2] = out[3] = nanv.f;
        return false;
    }
    const double n = (double)m[0], sx = (double)m[1], sy = (double)m[2], sz = (double)m[3];
    float cov[9];
    cov[0] = (float)(((double)m[4] - (sx * sx) / n) / n);
    cov[1] = (float)(((double)m[5] - (sx * sy) / n) / n);
    cov[2] = (float)(((double)m[6] - (sx * sz) / n) / n);
    cov[4] = (float)(((double)m[7] - (sy * sy) / n) / n);
    cov[5] = (float)(((double)m[8] - (sy * sz) / n) / n);
    cov[8] = (float)(((double)m[9] - (sz * sz) / n) / n);
    cov[3] = cov[1], cov[6] = cov[2], cov[7] = cov[5];
    pcl_plane_normal(cov, wx, wy, wz, out);
    return true;
}

}  // namespace dmsa
