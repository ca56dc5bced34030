// analytic_jacobian.hip — see analytic_jacobian.h.
//
// Mapping: one workgroup of four waves per Gaussian, the members in chunks of 64 (lane = member), chunk c to wave c mod 4.
//   * pass 1: the mean of the float global points p_j = T0[r_j] x_j (the correspondence kernels' transform), summed in fp64;
//   * pass 2: per member the 12-vector w (A + A^T) d_j (x) (x_j, 1) = ds/dT[r_j], added up per lane while the row stays the same (members of a
//     Gaussian come in ascending point index, so rows come in runs that span many chunks); where the row changes the wave sums the lanes'
//     12-vectors and contracts the sum ONCE with that row's 12 x P block of dT, lanes over theta (loop over blocks of 64 for P > 64), into
//     the wave's gradient in LDS.  (A cross-lane sum per chunk instead made the kernel 340 us on the bench window: the Gaussians of
//     thousands of members serialise on it.)
//   * the four wave gradients are added in wave order, scaled by sgn(s) / (2 e).
// Every sum runs in a fixed order (lane butterflies, then waves in order): no atomics, a call is bit-reproducible run to run.
#include "analytic_jacobian.h"
#include "wave_prims.h"

namespace dmsa {

namespace {

constexpr int kAjWaves = 4, kAjThreads = 64 * kAjWaves;

// the member's global point: its row of the table applied in the reference's order (apply_row3), as in the correspondence kernels
__device__ __forceinline__ float3 transform_member(const float4* __restrict__ table0, const float4 m) {
    const float4* t = table0 + (size_t)__float_as_int(m.w) * 3;
    return apply_row3(t[0], t[1], t[2], m.x, m.y, m.z);
}

__global__ __launch_bounds__(kAjThreads) void k_analytic_jacobian(const float4* __restrict__ memb, const int32_t* __restrict__ seg_off,
                                                                  const float4* __restrict__ info12, const float4* __restrict__ table0,
                                                                  const double* __restrict__ dT, int P, int id_row, double* __restrict__ E, int64_t ldE) {
    extern __shared__ double s_grad[];  // [kAjWaves][P]
    __shared__ double s_red[kAjWaves][4];
    const int g = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int off0 = seg_off[g], n = seg_off[g + 1] - off0;
    double* grad = s_grad + (size_t)wave * P;
    for (int k = lane; k < P; k += 64) grad[k] = 0.0;

    // pass 1: mean of the global points
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int i = threadIdx.x; i < n; i += kAjThreads) {
        const float3 p = transform_member(table0, memb[off0 + i]);
        sx += (double)p.x, sy += (double)p.y, sz += (double)p.z;
    }
    sx = wave_sum(sx), sy = wave_sum(sy), sz = wave_sum(sz);
    if (lane == 0) s_red[wave][0] = sx, s_red[wave][1] = sy, s_red[wave][2] = sz;
    __syncthreads();
    double mean[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) mean[a] = (((s_red[0][a] + s_red[1][a]) + s_red[2][a]) + s_red[3][a]) / (double)max(n, 1);

    // information matrix (column-major) and weight
    const float4 i0 = info12[3 * g], i1 = info12[3 * g + 1], i2 = info12[3 * g + 2];
    const double A[9] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w, i2.x};  // A[3 c + r] = A(r, c)
    const double w = i2.y;

    // pass 2.  acc: this lane's share of ds/dT[cur] since the last flush; `cur` (wave-uniform) changes -- and the wave reduces acc and contracts
    // it with the row's block of dT -- only where the row of the member sequence changes, not per chunk
    double s_part = 0.0;
    int cur = -1;
    double acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.0;
    auto flush = [&]() {
        double tot[12];
#pragma unroll
        for (int q = 0; q < 12; ++q) tot[q] = wave_sum(acc[q]), acc[q] = 0.0;
        const double* blk = dT + (size_t)cur * 12 * P;
        for (int k = lane; k < P; k += 64) {
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < 12; ++q) v += tot[q] * blk[(size_t)q * P + k];
            grad[k] += v;
        }
    };
    for (int c0 = wave * 64; c0 < n; c0 += kAjThreads) {
        const int i = c0 + lane;
        const bool on = i < n;
        int row = -1;
        double G[12];
#pragma unroll
        for (int q = 0; q < 12; ++q) G[q] = 0.0;
        if (on) {
            const float4 m = memb[off0 + i];
            row = __float_as_int(m.w);
            const float3 p = transform_member(table0, m);
            const double d[3] = {(double)p.x - mean[0], (double)p.y - mean[1], (double)p.z - mean[2]};
            double Ad[3], Atd[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                Ad[r] = A[r] * d[0] + A[3 + r] * d[1] + A[6 + r] * d[2];
                Atd[r] = A[3 * r] * d[0] + A[3 * r + 1] * d[1] + A[3 * r + 2] * d[2];
            }
            s_part += w * (d[0] * Ad[0] + d[1] * Ad[1] + d[2] * Ad[2]);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double wu = w * (Ad[r] + Atd[r]);
                G[4 * r] = wu * (double)m.x, G[4 * r + 1] = wu * (double)m.y, G[4 * r + 2] = wu * (double)m.z, G[4 * r + 3] = wu;
            }
        }
        const bool moves = on && row != id_row;  // static points: the identity row has no derivative
        unsigned long long pending = __ballot(moves);
        while (pending != 0ull) {  // wave-uniform: one round per distinct row of the chunk (ascending rows: the lowest lane's row first)
            const int leader = __ffsll((long long)pending) - 1;
            const int r = __shfl(row, leader);
            if (r != cur) {
                if (cur >= 0) flush();
                cur = r;
            }
            const bool mine = moves && row == r;
            pending &= ~__ballot(mine);
            if (mine) {
#pragma unroll
                for (int q = 0; q < 12; ++q) acc[q] += G[q];
            }
        }
    }
    if (cur >= 0) flush();
    s_part = wave_sum(s_part);
    if (lane == 0) s_red[wave][3] = s_part;
    __syncthreads();
    const double s = ((s_red[0][3] + s_red[1][3]) + s_red[2][3]) + s_red[3][3];
    const double e = sqrt(fabs(s));
    const double scale = e > 0.0 ? (s < 0.0 ? -0.5 : 0.5) / e : 0.0;
    for (int k = threadIdx.x; k < P; k += kAjThreads) {
        const double v = ((s_grad[k] + s_grad[P + k]) + s_grad[2 * P + k]) + s_grad[3 * P + k];
        E[(size_t)(k + 1) * ldE + g] = scale * v;
    }
}

}  // namespace

void launch_analytic_jacobian(const float4* memb_local, const int32_t* seg_off, const float* info12, const float* table0, const double* dT, int M, int P,
                              int id_row, double* E, int64_t ldE, hipStream_t s) {
    if (M <= 0 || P <= 0) return;
    hipLaunchKernelGGL(k_analytic_jacobian, dim3(M), dim3(kAjThreads), (size_t)kAjWaves * P * sizeof(double), s, memb_local, seg_off,
                       reinterpret_cast<const float4*>(info12), reinterpret_cast<const float4*>(table0), dT, P, id_row, E, ldE);
}

}  // namespace dmsa
