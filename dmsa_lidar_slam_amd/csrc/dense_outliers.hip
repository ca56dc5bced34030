// dense_outliers.hip — the kernels of include/dmsa_dense_outliers.h: statistical outlier removal for the dense cloud.
//
//   k_knn_mean_distance      O2-O3, the hot kernel: the traversal of csrc/dense_grid_walk.h with a per-lane list of the k smallest d2
//   k_outlier_quantise_sum   O4: q_i and the three exact int64 sums (a wave reduction, then plain 64-bit vector atomicAdd)
//   k_outlier_flags          O5's comparison, once the host has the threshold
//
// k_knn_mean_distance keeps each lane's list sorted, in registers: CAP floats touched only by fully unrolled loops with constant indices (no
// dynamically indexed private array, no scratch).  A candidate is first compared with the list's largest entry; the insertion network runs
// only when __ballot says some lane of the wave takes the candidate, and a lane that does not take it feeds the network +inf, which moves
// nothing.  After the first few tiles most candidates are rejected with that one compare.  The list holds values only (O3: a multiset), so
// equal distances need no rule, and the order in which the candidates arrive does not show in it.  The kernel is instantiated for
// capacities 4, 8 and 16 and launched with the smallest that holds k: the k smallest of all are the k smallest of the CAP smallest.
// Built with -ffp-contract=off.
#include "dense_outliers.h"

#include "dense_grid_walk.h"

#include <cmath>

namespace dmsa {
namespace {

template <int CAP>
__global__ __launch_bounds__(kBlock) void k_knn_mean_distance(const float4* __restrict__ pts, const uint32_t* __restrict__ idx, const unsigned long long* __restrict__ key,
                                                              const int64_t n, const DenseCellEntry* __restrict__ table, const uint32_t mask, const float r2,
                                                              const int32_t k, const int64_t first, const int64_t count, float* __restrict__ mean) {
    const int lane = threadIdx.x & 63;
    const int64_t self = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 64 + lane;  // this lane's sorted row
    bool live = self < n;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    int64_t row = 0;
    unsigned long long my_key = kCellEmptyKey;
    if (live) {
        row = (int64_t)idx[self] - first;
        live = row >= 0 && row < count;
    }
    if (live) {
        const float4 p = pts[self];
        qx = p.x, qy = p.y, qz = p.z;
        my_key = key[self];
    }
    if (__ballot(live) == 0ull) return;  // (the whole wave)
    float best[CAP];  // ascending; +inf = not filled (a candidate's d2 is at most r2)
#pragma unroll
    for (int s = 0; s < CAP; ++s) best[s] = INFINITY;
    const uint32_t me = (uint32_t)self;  // (n <= 2^26)
    d_walk_candidates(pts, n, table, mask, lane, live, my_key, [&](const bool mine, const float x, const float y, const float z, const uint32_t j) {
        const float dx = x - qx, dy = y - qy, dz = z - qz;
        float d2 = dx * dx;
        d2 += dy * dy;
        d2 += dz * dz;
        const bool take = mine && d2 <= r2 && j != me && d2 < best[CAP - 1];
        if (__ballot(take) != 0ull) {
            const float v = take ? d2 : INFINITY;
#pragma unroll
            for (int s = CAP - 1; s > 0; --s) best[s] = v < best[s - 1] ? best[s - 1] : (v < best[s] ? v : best[s]);  // (best[s - 1] is still the old one)
            best[0] = v < best[0] ? v : best[0];
        }
    });
    if (!live) return;
    float sum = 0.0f, kth = 0.0f;  // (0 + x is x)
#pragma unroll
    for (int s = 0; s < CAP; ++s)
        if (s < k) sum += __fsqrt_rn(best[s]), kth = best[s];
    mean[row] = kth <= r2 ? __fdiv_rn(sum, (float)k) : __int_as_float(0x7FC00000);
}

__global__ __launch_bounds__(kBlock) void k_outlier_quantise_sum(const float* __restrict__ mean, const int64_t n, const float scale, int32_t* __restrict__ q,
                                                                 unsigned long long* __restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long one = 0ull, s1 = 0ull, s2 = 0ull, iso = 0ull;
    if (i < n) {
        const float m = mean[i];
        int32_t qi = -1;
        if (m == m) {
            qi = (int32_t)rintf(m * scale);  // the product is exact; at most 2^18
            one = 1ull, s1 = (unsigned long long)qi, s2 = (unsigned long long)qi * (unsigned long long)qi;
        } else {
            iso = 1ull;
        }
        q[i] = qi;
    }
    one = wave_sum(one), s1 = wave_sum(s1), s2 = wave_sum(s2), iso = wave_sum(iso);
    if ((threadIdx.x & 63) == 0) {
        if (one != 0ull) atomicAdd(sums + OS_N, one), atomicAdd(sums + OS_S1, s1), atomicAdd(sums + OS_S2, s2);
        if (iso != 0ull) atomicAdd(sums + OS_ISOLATED, iso);
    }
}

__global__ __launch_bounds__(kBlock) void k_outlier_flags(const int32_t* __restrict__ q, const int64_t n, const double threshold, int32_t* __restrict__ keep,
                                                          uint8_t* __restrict__ flag8) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        keep[n] = 0;
        return;
    }
    const int32_t qi = q[i];
    const bool in = qi >= 0 && (double)qi <= threshold;
    keep[i] = in ? 1 : 0;
    flag8[i] = in ? 1 : 0;
}

}  // namespace

void launch_knn_mean_distance(const GridView& g, float r2, int32_t k, int64_t first, int64_t count, float* mean, hipStream_t s) {
    if (g.n <= 0 || count <= 0 || k < 1 || k > kOutlierMaxK) return;
    const auto kernel = k <= 4 ? k_knn_mean_distance<4> : k <= 8 ? k_knn_mean_distance<8> : k_knn_mean_distance<16>;  // the smallest capacity that holds k
    hipLaunchKernelGGL(kernel, dim3(blocks_for(g.n)), dim3(kBlock), 0, s, g.pts_sorted, g.idx_sorted, g.key_sorted, g.n, g.table, g.mask, r2, k, first, count, mean);
}
void launch_outlier_quantise_sum(const float* mean, int64_t n, float scale, int32_t* q, unsigned long long* sums, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_outlier_quantise_sum, dim3(blocks_for(n)), dim3(kBlock), 0, s, mean, n, scale, q, sums);
}
void launch_outlier_flags(const int32_t* q, int64_t n, double threshold, int32_t* keep, uint8_t* flag8, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_outlier_flags, dim3(blocks_for((unsigned long long)n + 1)), dim3(kBlock), 0, s, q, n, threshold, keep, flag8);
}

}  // namespace dmsa
