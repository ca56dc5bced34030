// dense_align.hip — the kernel of include/dmsa_dense_align.h: the dense cloud's reference aligned by ICP.
//
//   k_align_pair_sums         A2: from the completeness direction's best keys (k_nearest_across's output, the store row in the low word) the
//                             reference point and its store point, both quantised to int32, and the 25 exact int64 sums of a rigid fit
//
// The pattern of k_compare_quantise_sum: up to kAlignRows rows per lane in a grid-stride loop, a wave reduction, then one lane per wave adds
// its wave's 25 words to 25 words in LDS and, after the barrier, 25 lanes of the workgroup add those to HBM with plain 64-bit vector atomicAdd
// (words that are zero are not sent).  The products are integer, P * G in 64 bits from two 32-bit factors (v_mad_i64_i32's shape, as
// k_neighbour_moments); a float path through the quantised values would be wrong above 2^24.  Every accumulator is an unsigned 64-bit word:
// the sums are those of A2 modulo 2^64 and A2 bounds them below 2^58, so the words are the signed sums.  The accumulators are 25 named
// scalars, no private array, no scratch; every loop is bounded by n.  Built with -ffp-contract=off (p * scale_c is one exact product).
#include "dense_align.h"

#include "dense_dev.h"
#include "wave_prims.h"

#include <cmath>

namespace dmsa {
namespace {

constexpr int kAlignRows = 16;  // rows per lane, a launch's workgroups apart

struct CrossSum {
    unsigned long long lo = 0ull, hi = 0ull;
    __device__ __forceinline__ void add(const int32_t p, const int32_t g) {
        const long long prod = (long long)p * (long long)g;
        lo += (unsigned long long)(uint32_t)prod;
        hi += (unsigned long long)(prod >> 32);  // (arithmetic: hi * 2^32 + lo is the product)
    }
    __device__ __forceinline__ void reduce() { lo = wave_sum(lo), hi = wave_sum(hi); }
};

__device__ __forceinline__ int32_t d_quantise(const float v, const float scale_c) { return (int32_t)rintf(v * scale_c); }
__device__ __forceinline__ void d_lds_add(unsigned long long* acc, const int at, const unsigned long long v) {
    if (v != 0ull) atomicAdd(acc + at, v);
}

__global__ __launch_bounds__(kBlock) void k_align_pair_sums(const unsigned long long* __restrict__ best, const float4* __restrict__ ref_pts,
                                                            const uint8_t* __restrict__ ref_valid, const float4* __restrict__ store_pts, const int64_t store_rows,
                                                            const int64_t n, const float scale_c, unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long acc[kAlignSums];
    if (threadIdx.x < kAlignSums) acc[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long pairs = 0ull, px = 0ull, py = 0ull, pz = 0ull, gx = 0ull, gy = 0ull, gz = 0ull;
    CrossSum xx, xy, xz, yx, yy, yz, zx, zy, zz;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const unsigned long long k = best[i];
        const int64_t j = (int64_t)(uint32_t)k;
        if (k == kCompareNoMatch || ref_valid[i] == 0 || j >= store_rows) continue;  // (the last: never; a key holds a row of the store)
        const float4 p = ref_pts[i];
        const float4 g = store_pts[j];
        const int32_t Px = d_quantise(p.x, scale_c), Py = d_quantise(p.y, scale_c), Pz = d_quantise(p.z, scale_c);
        const int32_t Gx = d_quantise(g.x, scale_c), Gy = d_quantise(g.y, scale_c), Gz = d_quantise(g.z, scale_c);
        pairs += 1ull;
        px += (unsigned long long)(long long)Px, py += (unsigned long long)(long long)Py, pz += (unsigned long long)(long long)Pz;
        gx += (unsigned long long)(long long)Gx, gy += (unsigned long long)(long long)Gy, gz += (unsigned long long)(long long)Gz;
        xx.add(Px, Gx), xy.add(Px, Gy), xz.add(Px, Gz);
        yx.add(Py, Gx), yy.add(Py, Gy), yz.add(Py, Gz);
        zx.add(Pz, Gx), zy.add(Pz, Gy), zz.add(Pz, Gz);
    }
    pairs = wave_sum(pairs);
    if (pairs != 0ull) {  // (the same in all 64 lanes)
        px = wave_sum(px), py = wave_sum(py), pz = wave_sum(pz), gx = wave_sum(gx), gy = wave_sum(gy), gz = wave_sum(gz);
        xx.reduce(), xy.reduce(), xz.reduce(), yx.reduce(), yy.reduce(), yz.reduce(), zx.reduce(), zy.reduce(), zz.reduce();
        if ((threadIdx.x & 63) == 0) {
            d_lds_add(acc, 0, pairs);
            d_lds_add(acc, 1, px), d_lds_add(acc, 2, py), d_lds_add(acc, 3, pz), d_lds_add(acc, 4, gx), d_lds_add(acc, 5, gy), d_lds_add(acc, 6, gz);
            d_lds_add(acc, 7, xx.lo), d_lds_add(acc, 8, xx.hi), d_lds_add(acc, 9, xy.lo), d_lds_add(acc, 10, xy.hi), d_lds_add(acc, 11, xz.lo), d_lds_add(acc, 12, xz.hi);
            d_lds_add(acc, 13, yx.lo), d_lds_add(acc, 14, yx.hi), d_lds_add(acc, 15, yy.lo), d_lds_add(acc, 16, yy.hi), d_lds_add(acc, 17, yz.lo), d_lds_add(acc, 18, yz.hi);
            d_lds_add(acc, 19, zx.lo), d_lds_add(acc, 20, zx.hi), d_lds_add(acc, 21, zy.lo), d_lds_add(acc, 22, zy.hi), d_lds_add(acc, 23, zz.lo), d_lds_add(acc, 24, zz.hi);
        }
    }
    __syncthreads();
    if (threadIdx.x < kAlignSums && acc[threadIdx.x] != 0ull) atomicAdd(sums + threadIdx.x, acc[threadIdx.x]);
}

}  // namespace

void launch_align_pair_sums(const unsigned long long* best, const float4* ref_pts, const uint8_t* ref_valid, const float4* store_pts, int64_t store_rows, int64_t n,
                            float scale_c, unsigned long long* sums, hipStream_t s) {
    if (n > 0 && store_rows > 0)
        hipLaunchKernelGGL(k_align_pair_sums, dim3(blocks_for(((unsigned long long)n + kAlignRows - 1) / kAlignRows)), dim3(kBlock), 0, s, best, ref_pts, ref_valid,
                           store_pts, store_rows, n, scale_c, sums);
}

}  // namespace dmsa
