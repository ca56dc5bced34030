// dense_align.hip — the kernels of include/dmsa_dense_align.h and include/dmsa_dense_align_plane.h: the sums of a step of the dense cloud's
// reference aligned by ICP, point to point and point to plane.
//
//   k_align_pair_sums         A2: from the completeness direction's best keys (k_nearest_across's output, the store row in the low word) the
//                             reference point and its store point, both quantised to int32, and the 25 exact int64 sums of a rigid fit
//   k_align_plane_sums<Words> P1-P2: from the same keys the reference point, its store point and that row's normal, all three quantised to
//                             int32, and one group of the 64 exact int64 words of the step; launched once per group (LinearWords,
//                             SquareWords, ResidualWords)
//
// The pattern of k_compare_quantise_sum: up to kAlignRows rows per lane in a grid-stride loop, a wave reduction, then one lane per wave adds
// its wave's words to the kernel's words in LDS and, after the barrier, as many lanes of the workgroup add those to HBM with plain 64-bit
// vector atomicAdd (words that are zero are not sent).  Every product is integer: 32 x 32 -> 64 where A2's and P2's bounds allow it
// (v_mad_i64_i32's shape, as k_neighbour_moments; a float path through the quantised values would be wrong above 2^24), signed 64 x 64 ->
// 128 (__int128: the low product and the high-product instruction) for P2's c * c and c * e.  No float operation follows the quantisations.
// Every accumulator is an unsigned 64-bit word: the sums are those of A2 and P2 modulo 2^64 and both bound them below 2^58, so the words are
// the signed sums.  The accumulators are named scalars, alone or in small structs, no private array, no scratch; every loop is bounded by
// n.  Built with -ffp-contract=off (p * scale_c and n * 2^14 are exact products).
#include "dense_align.h"

#include "dense_dev.h"
#include "wave_prims.h"

#include <cmath>

namespace dmsa {
namespace {

constexpr int kAlignRows = 16;  // rows per lane, a launch's workgroups apart
typedef unsigned long long u64;

__device__ __forceinline__ void d_lds_add(u64* acc, const int at, const u64 v) {
    if (v != 0ull) atomicAdd(acc + at, v);
}

// A2's lo / hi form and P2's limb rule for a product below 2^63 in magnitude ...
struct Limbs2 {
    u64 l0 = 0ull, l1 = 0ull;
    __device__ __forceinline__ void add(const long long x) {
        l0 += (u64)(uint32_t)x;
        l1 += (u64)(x >> 32);  // (arithmetic: l1 * 2^32 + l0 is the product)
    }
    __device__ __forceinline__ void reduce() { l0 = wave_sum(l0), l1 = wave_sum(l1); }
    __device__ __forceinline__ void flush(u64* acc, const int at) const { d_lds_add(acc, at, l0), d_lds_add(acc, at + 1, l1); }
};
// ... and for one below 2^95
struct Limbs3 {
    u64 l0 = 0ull, l1 = 0ull, l2 = 0ull;
    __device__ __forceinline__ void add(const __int128 x) {
        l0 += (u64)(uint32_t)x;
        l1 += (u64)(uint32_t)(x >> 32);
        l2 += (u64)(long long)(x >> 64);  // (arithmetic)
    }
    __device__ __forceinline__ void reduce() { l0 = wave_sum(l0), l1 = wave_sum(l1), l2 = wave_sum(l2); }
    __device__ __forceinline__ void flush(u64* acc, const int at) const { d_lds_add(acc, at, l0), d_lds_add(acc, at + 1, l1), d_lds_add(acc, at + 2, l2); }
};

__device__ __forceinline__ int32_t d_quantise(const float v, const float scale) { return (int32_t)rintf(v * scale); }
// P1: a component of a normal that can be converted (false for NaN and infinity)
__device__ __forceinline__ bool d_normal_component(const float v) { return fabsf(v * 16384.0f) <= 32768.0f; }
__device__ __forceinline__ u64 d_word(const long long v) { return (u64)v; }

// whether reference row i is matched to a row of the store, *j
__device__ __forceinline__ bool d_matched_row(const int64_t i, const u64* __restrict__ best, const uint8_t* __restrict__ ref_valid, const int64_t store_rows, int64_t* j) {
    const u64 k = best[i];
    *j = (int64_t)(uint32_t)k;
    return k != kCompareNoMatch && ref_valid[i] != 0 && *j < store_rows;  // (the last: always; a key holds a row of the store)
}

__global__ __launch_bounds__(kBlock) void k_align_pair_sums(const u64* __restrict__ best, const float4* __restrict__ ref_pts, const uint8_t* __restrict__ ref_valid,
                                                            const float4* __restrict__ store_pts, const int64_t store_rows, const int64_t n, const float scale_c,
                                                            u64* __restrict__ sums) {
    __shared__ u64 acc[kAlignSums];
    if (threadIdx.x < kAlignSums) acc[threadIdx.x] = 0ull;
    __syncthreads();
    u64 pairs = 0ull, px = 0ull, py = 0ull, pz = 0ull, gx = 0ull, gy = 0ull, gz = 0ull;
    Limbs2 xx, xy, xz, yx, yy, yz, zx, zy, zz;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        int64_t j;
        if (!d_matched_row(i, best, ref_valid, store_rows, &j)) continue;
        const float4 p = ref_pts[i];
        const float4 g = store_pts[j];
        const long long Px = d_quantise(p.x, scale_c), Py = d_quantise(p.y, scale_c), Pz = d_quantise(p.z, scale_c);  // (32 x 32 -> 64 below)
        const long long Gx = d_quantise(g.x, scale_c), Gy = d_quantise(g.y, scale_c), Gz = d_quantise(g.z, scale_c);
        pairs += 1ull;
        px += d_word(Px), py += d_word(Py), pz += d_word(Pz), gx += d_word(Gx), gy += d_word(Gy), gz += d_word(Gz);
        xx.add(Px * Gx), xy.add(Px * Gy), xz.add(Px * Gz);
        yx.add(Py * Gx), yy.add(Py * Gy), yz.add(Py * Gz);
        zx.add(Pz * Gx), zy.add(Pz * Gy), zz.add(Pz * Gz);
    }
    pairs = wave_sum(pairs);
    if (pairs != 0ull) {  // (the same in all 64 lanes)
        px = wave_sum(px), py = wave_sum(py), pz = wave_sum(pz), gx = wave_sum(gx), gy = wave_sum(gy), gz = wave_sum(gz);
        xx.reduce(), xy.reduce(), xz.reduce(), yx.reduce(), yy.reduce(), yz.reduce(), zx.reduce(), zy.reduce(), zz.reduce();
        if ((threadIdx.x & 63) == 0) {
            d_lds_add(acc, 0, pairs);
            d_lds_add(acc, 1, px), d_lds_add(acc, 2, py), d_lds_add(acc, 3, pz), d_lds_add(acc, 4, gx), d_lds_add(acc, 5, gy), d_lds_add(acc, 6, gz);
            xx.flush(acc, 7), xy.flush(acc, 9), xz.flush(acc, 11), yx.flush(acc, 13), yy.flush(acc, 15), yz.flush(acc, 17), zx.flush(acc, 19), zy.flush(acc, 21), zz.flush(acc, 23);
        }
    }
    __syncthreads();
    if (threadIdx.x < kAlignSums && acc[threadIdx.x] != 0ull) atomicAdd(sums + threadIdx.x, acc[threadIdx.x]);
}

// P1-P2 of reference row i: whether it is matched, whether its store row has a normal, and the integers of the pair
struct PlanePair {
    bool matched = false, has = false;
    long long Px, Py, Pz, Nx, Ny, Nz, cx, cy, cz, e;
};
__device__ __forceinline__ PlanePair d_plane_pair(const int64_t i, const u64* __restrict__ best, const float4* __restrict__ ref_pts, const uint8_t* __restrict__ ref_valid,
                                                  const float4* __restrict__ store_pts, const float4* __restrict__ store_normals, const int64_t store_rows,
                                                  const float scale_c) {
    PlanePair q;
    int64_t j;
    if (!d_matched_row(i, best, ref_valid, store_rows, &j)) return q;
    q.matched = true;
    const float4 nv = store_normals[j];
    if (!(d_normal_component(nv.x) && d_normal_component(nv.y) && d_normal_component(nv.z))) return q;
    q.Nx = d_quantise(nv.x, 16384.0f), q.Ny = d_quantise(nv.y, 16384.0f), q.Nz = d_quantise(nv.z, 16384.0f);
    const long long len2 = q.Nx * q.Nx + q.Ny * q.Ny + q.Nz * q.Nz;
    if (len2 < (1ll << 27) || len2 > (1ll << 29)) return q;
    q.has = true;
    const float4 p = ref_pts[i];
    const float4 g = store_pts[j];
    q.Px = d_quantise(p.x, scale_c), q.Py = d_quantise(p.y, scale_c), q.Pz = d_quantise(p.z, scale_c);
    const long long Gx = d_quantise(g.x, scale_c), Gy = d_quantise(g.y, scale_c), Gz = d_quantise(g.z, scale_c);
    q.cx = q.Py * q.Nz - q.Pz * q.Ny, q.cy = q.Pz * q.Nx - q.Px * q.Nz, q.cz = q.Px * q.Ny - q.Py * q.Nx;  // |c| <= 2^45
    q.e = (Gx - q.Px) * q.Nx + (Gy - q.Py) * q.Ny + (Gz - q.Pz) * q.Nz;                                  // |e| < 2^31
    return q;
}

// The 64 words in three groups, each with the pattern's three steps: a pair added, the wave's sum, the wave's words into LDS (`acc` is the
// group's own block, its word 0 the word kFirst of P2's order).  One kernel cannot hold 64 words and their reduction in 256 VGPRs; each group
// can (profiles/r25_dense_align_resources.txt), so k_align_plane_sums runs once per group over the same pairs.
struct LinearWords {  // [0, 29): n, no_normal (the kernel's own), Sp, NN, cN
    static constexpr int kFirst = 0, kWords = 29;
    u64 px = 0ull, py = 0ull, pz = 0ull, nxx = 0ull, nxy = 0ull, nxz = 0ull, nyy = 0ull, nyz = 0ull, nzz = 0ull;
    Limbs2 cnxx, cnxy, cnxz, cnyx, cnyy, cnyz, cnzx, cnzy, cnzz;
    __device__ __forceinline__ void add(const PlanePair& q) {
        px += d_word(q.Px), py += d_word(q.Py), pz += d_word(q.Pz);
        nxx += d_word(q.Nx * q.Nx), nxy += d_word(q.Nx * q.Ny), nxz += d_word(q.Nx * q.Nz);
        nyy += d_word(q.Ny * q.Ny), nyz += d_word(q.Ny * q.Nz), nzz += d_word(q.Nz * q.Nz);
        cnxx.add(q.cx * q.Nx), cnxy.add(q.cx * q.Ny), cnxz.add(q.cx * q.Nz);
        cnyx.add(q.cy * q.Nx), cnyy.add(q.cy * q.Ny), cnyz.add(q.cy * q.Nz);
        cnzx.add(q.cz * q.Nx), cnzy.add(q.cz * q.Ny), cnzz.add(q.cz * q.Nz);
    }
    __device__ __forceinline__ void reduce() {
        px = wave_sum(px), py = wave_sum(py), pz = wave_sum(pz);
        nxx = wave_sum(nxx), nxy = wave_sum(nxy), nxz = wave_sum(nxz), nyy = wave_sum(nyy), nyz = wave_sum(nyz), nzz = wave_sum(nzz);
        cnxx.reduce(), cnxy.reduce(), cnxz.reduce(), cnyx.reduce(), cnyy.reduce(), cnyz.reduce(), cnzx.reduce(), cnzy.reduce(), cnzz.reduce();
    }
    __device__ __forceinline__ void flush(u64* acc) const {
        d_lds_add(acc, 2, px), d_lds_add(acc, 3, py), d_lds_add(acc, 4, pz);
        d_lds_add(acc, 5, nxx), d_lds_add(acc, 6, nxy), d_lds_add(acc, 7, nxz), d_lds_add(acc, 8, nyy), d_lds_add(acc, 9, nyz), d_lds_add(acc, 10, nzz);
        cnxx.flush(acc, 11), cnxy.flush(acc, 13), cnxz.flush(acc, 15), cnyx.flush(acc, 17), cnyy.flush(acc, 19), cnyz.flush(acc, 21);
        cnzx.flush(acc, 23), cnzy.flush(acc, 25), cnzz.flush(acc, 27);
    }
};
struct SquareWords {  // [29, 47): cc
    static constexpr int kFirst = 29, kWords = 18;
    Limbs3 xx, xy, xz, yy, yz, zz;
    __device__ __forceinline__ void add(const PlanePair& q) {
        xx.add((__int128)q.cx * q.cx), xy.add((__int128)q.cx * q.cy), xz.add((__int128)q.cx * q.cz);
        yy.add((__int128)q.cy * q.cy), yz.add((__int128)q.cy * q.cz), zz.add((__int128)q.cz * q.cz);
    }
    __device__ __forceinline__ void reduce() { xx.reduce(), xy.reduce(), xz.reduce(), yy.reduce(), yz.reduce(), zz.reduce(); }
    __device__ __forceinline__ void flush(u64* acc) const { xx.flush(acc, 0), xy.flush(acc, 3), xz.flush(acc, 6), yy.flush(acc, 9), yz.flush(acc, 12), zz.flush(acc, 15); }
};
struct ResidualWords {  // [47, 64): Ne, ce, ee
    static constexpr int kFirst = 47, kWords = 17;
    Limbs2 nex, ney, nez, ee;
    Limbs3 cex, cey, cez;
    __device__ __forceinline__ void add(const PlanePair& q) {
        nex.add(q.Nx * q.e), ney.add(q.Ny * q.e), nez.add(q.Nz * q.e);
        cex.add((__int128)q.cx * q.e), cey.add((__int128)q.cy * q.e), cez.add((__int128)q.cz * q.e);
        ee.add(q.e * q.e);
    }
    __device__ __forceinline__ void reduce() { nex.reduce(), ney.reduce(), nez.reduce(), cex.reduce(), cey.reduce(), cez.reduce(), ee.reduce(); }
    __device__ __forceinline__ void flush(u64* acc) const {
        nex.flush(acc, 0), ney.flush(acc, 2), nez.flush(acc, 4), cex.flush(acc, 6), cey.flush(acc, 9), cez.flush(acc, 12), ee.flush(acc, 15);
    }
};

template <class Words>
__global__ __launch_bounds__(kBlock) void k_align_plane_sums(const u64* __restrict__ best, const float4* __restrict__ ref_pts, const uint8_t* __restrict__ ref_valid,
                                                             const float4* __restrict__ store_pts, const float4* __restrict__ store_normals, const int64_t store_rows,
                                                             const int64_t n, const float scale_c, u64* __restrict__ sums) {
    constexpr bool kCounts = Words::kFirst == 0;  // the group that holds n and no_normal
    __shared__ u64 acc[Words::kWords];
    if (threadIdx.x < Words::kWords) acc[threadIdx.x] = 0ull;
    __syncthreads();
    u64 used = 0ull, bare = 0ull;
    Words w;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const PlanePair q = d_plane_pair(i, best, ref_pts, ref_valid, store_pts, store_normals, store_rows, scale_c);
        if (!q.matched) continue;
        if (!q.has) {
            bare += 1ull;
            continue;
        }
        used += 1ull;
        w.add(q);
    }
    const bool lane0 = (threadIdx.x & 63) == 0;
    used = wave_sum(used);
    if (kCounts) {
        bare = wave_sum(bare);
        if (lane0) d_lds_add(acc, 0, used), d_lds_add(acc, 1, bare);
    }
    if (used != 0ull) {  // (the same in all 64 lanes)
        w.reduce();
        if (lane0) w.flush(acc);
    }
    __syncthreads();
    if (threadIdx.x < Words::kWords && acc[threadIdx.x] != 0ull) atomicAdd(sums + Words::kFirst + threadIdx.x, acc[threadIdx.x]);
}

// a launch's workgroups: kAlignRows reference rows per lane
dim3 align_grid(const int64_t n) { return dim3(blocks_for(((unsigned long long)n + kAlignRows - 1) / kAlignRows)); }

}  // namespace

void launch_align_pair_sums(const unsigned long long* best, const float4* ref_pts, const uint8_t* ref_valid, const float4* store_pts, int64_t store_rows, int64_t n,
                            float scale_c, unsigned long long* sums, hipStream_t s) {
    if (n < 1 || store_rows < 1) return;
    hipLaunchKernelGGL(k_align_pair_sums, align_grid(n), dim3(kBlock), 0, s, best, ref_pts, ref_valid, store_pts, store_rows, n, scale_c, sums);
}

void launch_align_plane_sums(const unsigned long long* best, const float4* ref_pts, const uint8_t* ref_valid, const float4* store_pts, const float4* store_normals,
                             int64_t store_rows, int64_t n, float scale_c, unsigned long long* sums, hipStream_t s) {
    static_assert(LinearWords::kWords + SquareWords::kWords + ResidualWords::kWords == kAlignPlaneSums, "the three groups are the 64 words");
    if (n < 1 || store_rows < 1) return;
    const dim3 grid = align_grid(n);
    hipLaunchKernelGGL(k_align_plane_sums<LinearWords>, grid, dim3(kBlock), 0, s, best, ref_pts, ref_valid, store_pts, store_normals, store_rows, n, scale_c, sums);
    hipLaunchKernelGGL(k_align_plane_sums<SquareWords>, grid, dim3(kBlock), 0, s, best, ref_pts, ref_valid, store_pts, store_normals, store_rows, n, scale_c, sums);
    hipLaunchKernelGGL(k_align_plane_sums<ResidualWords>, grid, dim3(kBlock), 0, s, best, ref_pts, ref_valid, store_pts, store_normals, store_rows, n, scale_c, sums);
}

}  // namespace dmsa
