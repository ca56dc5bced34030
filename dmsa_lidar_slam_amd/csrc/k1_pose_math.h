// k1_pose_math.h — the fp64 rotation helpers of K1 (dense pose tables), stated once for the kernel files that interpolate poses:
// dmsa_kernels.hip (the window's dense pose tables) and dense_cloud.hip (one pose per raw point).  sin / cos / acos / atan2 come from
// include/dmsa_detmath.h: fixed sequences of correctly rounded IEEE operations, so the results are bit-identical to the host's and the
// oracle's.  Device-only, everything __forceinline__ (as wave_prims.h): a kernel compiles to the same instructions as with the helper
// written out beside it.  Build with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#include "../../include/dmsa_detmath.h"

namespace dmsa {

struct D3 {
    double x, y, z;
};
// kCut = false: the derivative side (k_*_pose_table_deriv), as so3_exp<false> of pose_math.h -- no identity cut at 1e-5
template <bool kCut = true>
__device__ __forceinline__ void d_so3_exp(const D3 w, double R[9]) {
    const double theta = sqrt(w.x * w.x + w.y * w.y + w.z * w.z);
    if (kCut ? theta < 0.00001 : theta * theta == 0.0) {
        R[0] = 1, R[1] = 0, R[2] = 0, R[3] = 0, R[4] = 1, R[5] = 0, R[6] = 0, R[7] = 0, R[8] = 1;
        return;
    }
    const double s = dmsa_det::det_sin(theta) / theta;
    const double sh = dmsa_det::det_sin(0.5 * theta);
    const double c = 2.0 * sh * sh / (theta * theta);
    const double t2 = theta * theta;
    R[0] = 1.0 + c * (w.x * w.x - t2);
    R[4] = 1.0 + c * (w.y * w.y - t2);
    R[8] = 1.0 + c * (w.z * w.z - t2);
    R[1] = c * w.x * w.y - s * w.z;
    R[3] = c * w.x * w.y + s * w.z;
    R[2] = c * w.x * w.z + s * w.y;
    R[6] = c * w.x * w.z - s * w.y;
    R[5] = c * w.y * w.z - s * w.x;
    R[7] = c * w.y * w.z + s * w.x;
}
__device__ __forceinline__ void d_quat_from_axang(const D3 a, double q[4]) {
    const double sq = a.x * a.x + a.y * a.y + a.z * a.z;
    const double ang = sqrt(sq);
    D3 ax = a;
    if (sq > 0.0) ax = D3{a.x / ang, a.y / ang, a.z / ang};
    const double sh = dmsa_det::det_sin(0.5 * ang);
    q[0] = dmsa_det::det_cos(0.5 * ang), q[1] = sh * ax.x, q[2] = sh * ax.y, q[3] = sh * ax.z;
}
// slerp of two rotations given as the unit quaternions d_quat_from_axang makes of them (helpers.h:24-37)
__device__ __forceinline__ D3 d_slerp_quat(const double* q1, const double* q2, const double t) {
    const double one = 1.0 - DBL_EPSILON;
    const double d = q1[0] * q2[0] + q1[1] * q2[1] + q1[2] * q2[2] + q1[3] * q2[3];
    const double ad = fabs(d);
    double s0, s1;
    if (ad >= one) {
        s0 = 1.0 - t, s1 = t;
    } else {
        const double th = dmsa_det::det_acos(ad), sn = dmsa_det::det_sin(th);
        s0 = dmsa_det::det_sin((1.0 - t) * th) / sn;
        s1 = dmsa_det::det_sin(t * th) / sn;
    }
    if (d < 0.0) s1 = -s1;
    const double qw = s0 * q1[0] + s1 * q2[0], qx = s0 * q1[1] + s1 * q2[1], qy = s0 * q1[2] + s1 * q2[2], qz = s0 * q1[3] + s1 * q2[3];
    double n = sqrt(qx * qx + qy * qy + qz * qz);
    if (n == 0.0) return D3{0.0, 0.0, 0.0};
    const double angle = 2.0 * dmsa_det::det_atan2(n, fabs(qw));
    if (qw < 0.0) n = -n;
    return D3{(qx / n) * angle, (qy / n) * angle, (qz / n) * angle};
}

}  // namespace dmsa
