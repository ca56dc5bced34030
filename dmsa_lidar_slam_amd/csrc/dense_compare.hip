// dense_compare.hip — the kernels of include/dmsa_dense_compare.h: the dense cloud against a reference cloud.
//
//   k_reference_transform     D0: the alignment in rule 5's form, and which rows are valid
//   k_reference_cell_keys     the cell keys of the reference's own search grid; an invalid row's key sorts it behind every valid row
//   k_nearest_across          D2, the hot kernel: the traversal of csrc/dense_grid_walk.h with the QUERIES of one grid and the TABLE and sorted
//                             points of the other; one 64-bit best key per lane
//   k_compare_quantise_sum    D2's dist and index, D4: q_i, the exact int64 sums (several rows per lane, a wave reduction, then plain 64-bit
//                             vector atomicAdd) and the histogram (counted in LDS per workgroup, then one atomicAdd per bin that is not empty)
//   k_compare_flags           D6's flags
//
// k_nearest_across: both grids are cut with the same edge, so a query's cell key names the same cell in the other set's table, and the
// walker needs nothing new: it is handed the other set's table and points and this set's keys.  A lane's state is one 64-bit key,
// (bits(d2) << 32) | original row, in two registers; a minimum over such keys does not depend on the order the candidates arrive in (D2).
// The candidate's original row is a load from idx_sorted at an address that is the same in all 64 lanes, and it is issued only when
// __ballot says some lane's d2 does not lose to its best: after the first tiles that is rare.  No private array, no scratch, no LDS, every
// loop bound the walker's.  Built with -ffp-contract=off (D2 is N2's expression, operation for operation).
#include "dense_compare.h"

#include "dense_grid_walk.h"

#include <cmath>

namespace dmsa {
namespace {

constexpr int kCompareSumRows = 16;  // rows per lane of k_compare_quantise_sum, a launch's workgroups apart

__global__ __launch_bounds__(kBlock) void k_reference_transform(const float* __restrict__ raw, const int64_t n, const int32_t stride, const bool transform,
                                                                const RefTransform T, const float voxel_size, float4* __restrict__ pts, uint8_t* __restrict__ valid,
                                                                unsigned long long* __restrict__ invalid) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long bad = 0ull;
    if (i < n) {
        const float* r = raw + i * (int64_t)stride;
        float3 g = make_float3(r[0], r[1], r[2]);
        if (transform)
            g = apply_row3(make_float4(T.c[0], T.c[1], T.c[2], T.c[3]), make_float4(T.c[4], T.c[5], T.c[6], T.c[7]), make_float4(T.c[8], T.c[9], T.c[10], T.c[11]), g.x,
                           g.y, g.z);
        // rule 6's bound (a NaN or an infinity fails it as it fails isfinite: floorf keeps either)
        const float cx = floorf(g.x / voxel_size), cy = floorf(g.y / voxel_size), cz = floorf(g.z / voxel_size);
        const float lim = 1048576.0f;  // 2^20
        const bool ok = isfinite(g.x) && isfinite(g.y) && isfinite(g.z) && cx >= -lim && cx < lim && cy >= -lim && cy < lim && cz >= -lim && cz < lim;
        pts[i] = make_float4(g.x, g.y, g.z, 0.0f);
        valid[i] = ok ? 1 : 0;
        bad = ok ? 0ull : 1ull;
    }
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad != 0ull) atomicAdd(invalid, bad);
}

// (the expression of k_grid_cell_keys: the cells are cut in double)
__device__ __forceinline__ int d_ref_cell_axis(const float v, const double cell) {
    const double c = floor((double)v / cell);
    return (int)fmin(fmax(c, -1048576.0), 1048575.0) + kCellBias;
}
__global__ __launch_bounds__(kBlock) void k_reference_cell_keys(const float4* __restrict__ pts, const uint8_t* __restrict__ valid, const int64_t n, const double cell,
                                                                unsigned long long* __restrict__ key, uint32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    key[i] = valid[i] ? d_cell_key(d_ref_cell_axis(p.x, cell), d_ref_cell_axis(p.y, cell), d_ref_cell_axis(p.z, cell)) : kCellEmptyKey;
    idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_nearest_across(const float4* __restrict__ q_pts, const uint32_t* __restrict__ q_idx, const unsigned long long* __restrict__ q_key,
                                                           const int64_t nq, const float4* __restrict__ s_pts, const uint32_t* __restrict__ s_idx, const int64_t ns,
                                                           const DenseCellEntry* __restrict__ s_table, const uint32_t s_mask, const float r2, const int64_t first,
                                                           const int64_t count, unsigned long long* __restrict__ best_out) {
    const int lane = threadIdx.x & 63;
    const int64_t self = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 64 + lane;  // this lane's sorted row of the query set
    bool live = self < nq;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    int64_t row = 0;
    unsigned long long my_key = kCellEmptyKey;
    if (live) {
        row = (int64_t)q_idx[self] - first;
        live = row >= 0 && row < count;
    }
    if (live) {
        const float4 p = q_pts[self];
        qx = p.x, qy = p.y, qz = p.z;
        my_key = q_key[self];
    }
    if (__ballot(live) == 0ull) return;  // (the whole wave)
    unsigned long long best = kCompareNoMatch;
    d_walk_candidates(s_pts, ns, s_table, s_mask, lane, live, my_key, [&](const bool mine, const float x, const float y, const float z, const uint32_t j) {
        const float dx = x - qx, dy = y - qy, dz = z - qz;
        float d2 = dx * dx;
        d2 += dy * dy;
        d2 += dz * dz;
        const uint32_t bits = __float_as_uint(d2);  // (d2 >= +0: it orders as its bits)
        const bool take = mine && d2 <= r2 && bits <= (uint32_t)(best >> 32);
        if (__ballot(take) != 0ull) {
            const unsigned long long k = ((unsigned long long)bits << 32) | (unsigned long long)s_idx[j];  // (j < ns, the same in every lane)
            if (take && k < best) best = k;
        }
    });
    if (live) best_out[row] = best;
}

__global__ __launch_bounds__(kBlock) void k_compare_quantise_sum(const unsigned long long* __restrict__ best, const uint8_t* __restrict__ valid, const int64_t n,
                                                                 const float scale, const uint32_t tol_bits, float* __restrict__ dist, int32_t* __restrict__ index,
                                                                 unsigned long long* __restrict__ sums) {
    __shared__ uint32_t bins[64];
    if (threadIdx.x < 64) bins[threadIdx.x] = 0u;
    __syncthreads();
    // up to kCompareSumRows rows per lane (a grid-stride loop) before the reduction: the atomics below go to the same few words from every
    // wave, and their number is what this kernel would otherwise wait for
    unsigned long long one = 0ull, s1 = 0ull, s2 = 0ull, none = 0ull, within = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const unsigned long long k = best[i];
        const bool counted = valid == nullptr || valid[i] != 0;
        float d = __int_as_float(0x7FC00000);
        int32_t at = -1;
        if (k != kCompareNoMatch) {
            const uint32_t bits = (uint32_t)(k >> 32);
            d = sqrtf(__uint_as_float(bits));  // correctly rounded (the compiler's default for sqrtf in device code; __fsqrt_rn was an ulp off here)
            at = (int32_t)(uint32_t)k;
            const int32_t qi = (int32_t)rintf(d * scale);  // the product is exact; at most 2^18
            one += 1ull, s1 += (unsigned long long)qi, s2 += (unsigned long long)qi * (unsigned long long)qi;
            within += bits <= tol_bits ? 1ull : 0ull;
            atomicAdd(&bins[min(qi >> 12, 63)], 1u);  // (at most 2^26 rows in all: a bin fits 32 bits)
        } else if (counted) {
            none += 1ull;
        }
        dist[i] = d, index[i] = at;
    }
    one = wave_sum(one), s1 = wave_sum(s1), s2 = wave_sum(s2), none = wave_sum(none), within = wave_sum(within);
    if ((threadIdx.x & 63) == 0) {
        if (one != 0ull) atomicAdd(sums + CM_MATCHED, one), atomicAdd(sums + CM_S1, s1), atomicAdd(sums + CM_S2, s2);
        if (none != 0ull) atomicAdd(sums + CM_UNMATCHED, none);
        if (within != 0ull) atomicAdd(sums + CM_WITHIN, within);
    }
    __syncthreads();
    if (threadIdx.x < 64 && bins[threadIdx.x] != 0u) atomicAdd(sums + CM_BINS + threadIdx.x, (unsigned long long)bins[threadIdx.x]);
}

__global__ __launch_bounds__(kBlock) void k_compare_flags(const unsigned long long* __restrict__ best, const int64_t n, const uint32_t tol_bits, const bool near,
                                                          int32_t* __restrict__ keep, uint8_t* __restrict__ flag8, unsigned long long* __restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long kept = 0ull;
    if (i < n) {
        const unsigned long long k = best[i];
        const bool confirmed = k != kCompareNoMatch && (uint32_t)(k >> 32) <= tol_bits;
        const bool in = confirmed == near;
        keep[i] = in ? 1 : 0;
        flag8[i] = in ? 1 : 0;
        kept = in ? 1ull : 0ull;
    } else if (i == n) {
        keep[n] = 0;
    }
    kept = wave_sum(kept);
    if ((threadIdx.x & 63) == 0 && kept != 0ull) atomicAdd(sums + CM_KEPT, kept);
}

}  // namespace

void launch_reference_transform(const float* raw, int64_t n, int32_t stride_floats, bool transform, RefTransform T, float voxel_size, float4* pts, uint8_t* valid,
                                unsigned long long* invalid, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_reference_transform, dim3(blocks_for(n)), dim3(kBlock), 0, s, raw, n, stride_floats, transform, T, voxel_size, pts, valid, invalid);
}
void launch_reference_cell_keys(const float4* pts, const uint8_t* valid, int64_t n, double cell, unsigned long long* key, uint32_t* idx, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_reference_cell_keys, dim3(blocks_for(n)), dim3(kBlock), 0, s, pts, valid, n, cell, key, idx);
}
void launch_nearest_across(const GridView& q, const GridView& in, float r2, int64_t first, int64_t count, unsigned long long* best, hipStream_t s) {
    if (q.n <= 0 || in.n <= 0 || count <= 0) return;
    hipLaunchKernelGGL(k_nearest_across, dim3(blocks_for(q.n)), dim3(kBlock), 0, s, q.pts_sorted, q.idx_sorted, q.key_sorted, q.n, in.pts_sorted, in.idx_sorted, in.n,
                       in.table, in.mask, r2, first, count, best);
}
void launch_compare_quantise_sum(const unsigned long long* best, const uint8_t* valid, int64_t n, float scale, uint32_t tol_bits, float* dist, int32_t* index,
                                 unsigned long long* sums, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_compare_quantise_sum, dim3(blocks_for(((unsigned long long)n + kCompareSumRows - 1) / kCompareSumRows)), dim3(kBlock), 0, s, best, valid, n, scale, tol_bits, dist, index, sums);
}
void launch_compare_flags(const unsigned long long* best, int64_t n, uint32_t tol_bits, bool near, int32_t* keep, uint8_t* flag8, unsigned long long* sums,
                          hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_compare_flags, dim3(blocks_for((unsigned long long)n + 1)), dim3(kBlock), 0, s, best, n, tol_bits, near, keep, flag8, sums);
}

}  // namespace dmsa
