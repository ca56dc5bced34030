// analytic_jacobian.h — the point-to-Gaussian rows of the Jacobian from the pose-table derivatives (settings.use_analytic_jacobi != 0).
// For Gaussian k with members j (DmsaOptimizer.h:234-273): s_k = w_k sum_j d_j^T A_k d_j, d_j = p_j - m_k, e_k = sqrt|s_k|; the mean's own
// derivative drops out (sum_j d_j = 0), so
//     de_k/dtheta = sgn(s_k) w_k / (2 e_k) sum_j ((A_k + A_k^T) d_j)^T (dR_{r_j}/dtheta x_j + dt_{r_j}/dtheta)
// with x_j the local point and r_j its pose-table row; the identity row of the static points contributes nothing, e_k = 0 gives a zero row.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dmsa {

// Largest P the kernel takes (its per-wave partial gradients live in LDS: 4 x P doubles).
constexpr int kAnalyticJacobianMaxP = 2040;
// memb_local / seg_off / info12: the Gaussians as the correspondence kernels read them; table0: the evaluation-0 pose table ([row][12] floats);
// dT: [rows][12][P] doubles (launch_*_pose_table_deriv); id_row: the identity row.  Writes E[(k + 1) * ldE + g] = de_g/dtheta_k for g < M.
void launch_analytic_jacobian(const float4* memb_local, const int32_t* seg_off, const float* info12, const float* table0, const double* dT, int M, int P,
                              int id_row, double* E, int64_t ldE, hipStream_t s);

}  // namespace dmsa
