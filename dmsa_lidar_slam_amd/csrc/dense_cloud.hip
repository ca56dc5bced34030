// dense_cloud.hip — the kernels of include/dmsa_dense_cloud.h: every raw point of a scan placed at the pose interpolated for its own stamp.
//
//   k_dense_interpolate   rules 3-4 for a list of stamps (the stage call the tests stand on)
//   k_dense_place         rules 1-6: gates, segment, fp64 slerp + exponential (k1_pose_math.h), float transform, voxel key
//   k_voxel_claim / k_voxel_resolve / k_voxel_rollback / k_voxel_rehash   the cross-scan voxel set, an open-addressing table in HBM
//   k_dense_scatter / k_dense_pack_rows   stable compaction (the scan is the library's exclusive_scan_i32) and the 12- or 16-byte file rows
//
// One thread per point throughout; the fp64 work per point is one slerp and one exponential.  Built with -ffp-contract=off like every
// file here: rule 4 wants every fp64 operation rounded on its own, rule 5 the float transform in apply_row3's order.
#include "dense_cloud.h"

#include "dense_dev.h"
#include "k1_pose_math.h"
#include "wave_prims.h"

#include <cmath>

namespace dmsa {
namespace {

constexpr unsigned long long kEmpty = ~0ull;

// the largest j in [lo, hi] with s[j] <= t, given s[lo] <= t.  hi - lo < 2^31, so 32 halvings always suffice: the bound is never what ends it
__device__ __forceinline__ int d_find_segment(const double* s, int lo, int hi, const double t) {
#pragma unroll 1
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        if (s[mid] <= t)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// rules 3 (gap) and 4 for a stamp t inside segment k of the arrays s / p / q (global memory or a workgroup's LDS copy): false = in a gap.
// The one body both kernels run.
__device__ __forceinline__ bool d_dense_pose(const double* s, const double* p, const double* q, const int k, const double t, const double max_gap, double R[9],
                                             double tr[3]) {
    const double s0 = s[k];
    const double ds = s[k + 1] - s0;
    if (max_gap > 0.0 && ds > max_gap) return false;
    const double u = (t - s0) / ds;
    const D3 o = d_slerp_quat(&q[4 * k], &q[4 * (k + 1)], u);
    d_so3_exp(o, R);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double p0 = p[3 * k + a];
        const double d = p[3 * (k + 1) + a] - p0;
        tr[a] = p0 + u * d;
    }
    return true;
}

__global__ __launch_bounds__(kBlock) void k_dense_interpolate(const DenseTraj tj, const double max_gap, const double* __restrict__ ts, const int64_t n,
                                                              double* __restrict__ pose12, int32_t* __restrict__ segment) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double t = ts[i];
    double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, tr[3] = {0, 0, 0};
    int seg = -1;
    if (t >= tj.stamps[0] && t <= tj.stamps[tj.n_p - 1]) {  // (a NaN compares false)
        seg = d_find_segment(tj.stamps, 0, tj.n_p - 2, t);
        if (!d_dense_pose(tj.stamps, tj.pos, tj.quat, seg, t, max_gap, R, tr)) {
            seg = -2;
            for (int k = 0; k < 9; ++k) R[k] = 0.0;
        }
    }
    if (pose12) {
        for (int k = 0; k < 9; ++k) pose12[12 * i + k] = R[k];
        for (int k = 0; k < 3; ++k) pose12[12 * i + 9 + k] = tr[k];
    }
    if (segment) segment[i] = seg;
}

// A scan spans about 0.1 s and its points come in time order, so the 256 points of a workgroup touch one or two trajectory segments.  The
// workgroup reduces the stamp bounds of its live points, one thread finds their segment range in the global stamps, and when the range
// fits (kDensePoseLds poses) those poses are staged in LDS; every thread then searches its segment inside that range only.  A workgroup
// whose stamps span more (an unordered scan) searches the same range in global memory: same arithmetic on the same numbers, same bits.
// kIntensity (include/dmsa_dense_intensity.h, I3): the fourth float of a placed point is the input row's, bit for bit, instead of 1; no rule reads it.
template <bool kIntensity>
__global__ __launch_bounds__(kBlock) void k_dense_place(const float4* __restrict__ xyz, const double* __restrict__ stamps, const int64_t n, const DenseTraj tj,
                                                        const DenseGates gt, float4* __restrict__ placed, int32_t* __restrict__ keep,
                                                        unsigned long long* __restrict__ key, unsigned long long* __restrict__ counters, float4* __restrict__ origin) {
    __shared__ double s_stamp[kDensePoseLds], s_pos[3 * kDensePoseLds], s_quat[4 * kDensePoseLds];
    __shared__ double s_min[kBlock / 64], s_max[kBlock / 64];
    __shared__ int s_lo, s_hi;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double first = tj.stamps[0], last = tj.stamps[tj.n_p - 1];
    int code = -1;  // -1 no point, 0 live, 1 + DenseCounter: dropped
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    double t = 0.0;
    if (i < n) {
        p = xyz[i];
        const double ti = stamps[i];
        code = 0;
        if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(ti))) {
            code = 1 + DC_NON_FINITE;
        } else {
            const float xx = p.x * p.x, yy = p.y * p.y, zz = p.z * p.z;
            const float yz = yy + zz;
            const float r = sqrtf(xx + yz);
            if (!(r > gt.min_range && (gt.max_range <= 0.0f || r < gt.max_range))) {
                code = 1 + DC_OUT_OF_RANGE;
            } else {
                t = ti + gt.time_offset;
                if (!(t >= first && t <= last)) code = 1 + DC_OUT_OF_TIME;
            }
        }
    }
    // stamp bounds of the workgroup's live points
    double mn = code == 0 ? t : INFINITY, mx = code == 0 ? t : -INFINITY;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = fmin(mn, __shfl_xor(mn, o)), mx = fmax(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = mn, s_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) mn = fmin(mn, s_min[w]), mx = fmax(mx, s_max[w]);
        int lo = 0, hi = -1;  // hi < lo: no live point
        if (mn <= mx) {
            lo = d_find_segment(tj.stamps, 0, tj.n_p - 2, mn);
            hi = d_find_segment(tj.stamps, lo, tj.n_p - 2, mx);
        }
        s_lo = lo, s_hi = hi;
    }
    __syncthreads();
    const int lo = s_lo, hi = s_hi;
    const int poses = hi - lo + 2;  // poses lo .. hi + 1
    const bool in_lds = poses <= kDensePoseLds;
    if (in_lds && hi >= lo) {
        if ((int)threadIdx.x < poses) s_stamp[threadIdx.x] = tj.stamps[lo + threadIdx.x];
        if ((int)threadIdx.x < 3 * poses) s_pos[threadIdx.x] = tj.pos[3 * lo + threadIdx.x];
        if ((int)threadIdx.x < 4 * poses) s_quat[threadIdx.x] = tj.quat[4 * lo + threadIdx.x];
    }
    __syncthreads();
    float3 g = make_float3(0.0f, 0.0f, 0.0f), org = make_float3(0.0f, 0.0f, 0.0f);
    unsigned long long vk = kEmpty;
    if (code == 0) {
        const double* S = in_lds ? s_stamp : tj.stamps + lo;
        const double* P = in_lds ? s_pos : tj.pos + 3 * (size_t)lo;
        const double* Q = in_lds ? s_quat : tj.quat + 4 * (size_t)lo;
        const int k = d_find_segment(S, 0, hi - lo, t);
        double R[9], tr[3];
        if (!d_dense_pose(S, P, Q, k, t, gt.max_pose_gap, R, tr)) {
            code = 1 + DC_IN_GAP;
        } else {
            const float3 q = apply_row3(make_float4(gt.l2i[0], gt.l2i[1], gt.l2i[2], gt.l2i[3]), make_float4(gt.l2i[4], gt.l2i[5], gt.l2i[6], gt.l2i[7]),
                                        make_float4(gt.l2i[8], gt.l2i[9], gt.l2i[10], gt.l2i[11]), p.x, p.y, p.z);
            g = apply_row3(make_float4((float)R[0], (float)R[1], (float)R[2], (float)tr[0]), make_float4((float)R[3], (float)R[4], (float)R[5], (float)tr[1]),
                           make_float4((float)R[6], (float)R[7], (float)R[8], (float)tr[2]), q.x, q.y, q.z);
            if (origin) {  // where the sensor stood when this point was measured: the same two transforms for the sensor-frame point (0, 0, 0)
                const float3 q0 = apply_row3(make_float4(gt.l2i[0], gt.l2i[1], gt.l2i[2], gt.l2i[3]), make_float4(gt.l2i[4], gt.l2i[5], gt.l2i[6], gt.l2i[7]),
                                             make_float4(gt.l2i[8], gt.l2i[9], gt.l2i[10], gt.l2i[11]), 0.0f, 0.0f, 0.0f);
                org = apply_row3(make_float4((float)R[0], (float)R[1], (float)R[2], (float)tr[0]), make_float4((float)R[3], (float)R[4], (float)R[5], (float)tr[1]),
                                 make_float4((float)R[6], (float)R[7], (float)R[8], (float)tr[2]), q0.x, q0.y, q0.z);
            }
            if (gt.voxel_size > 0.0f) {
                const float cx = floorf(g.x / gt.voxel_size), cy = floorf(g.y / gt.voxel_size), cz = floorf(g.z / gt.voxel_size);
                const float lim = 1048576.0f;  // 2^20
                if (!(cx >= -lim && cx < lim && cy >= -lim && cy < lim && cz >= -lim && cz < lim)) {
                    code = 1 + DC_OUT_OF_GRID;
                } else {
                    const unsigned long long bx = (unsigned long long)((int)cx + 1048576), by = (unsigned long long)((int)cy + 1048576),
                                             bz = (unsigned long long)((int)cz + 1048576);
                    vk = (bx << 42) | (by << 21) | bz;
                }
            }
        }
    }
    if (i < n) {
        placed[i] = make_float4(g.x, g.y, g.z, kIntensity ? p.w : 1.0f);
        if (origin) origin[i] = make_float4(org.x, org.y, org.z, 1.0f);
        keep[i] = code == 0 ? 1 : 0;
        key[i] = code == 0 ? vk : kEmpty;
        if (code > 0) atomicAdd(&counters[code - 1], 1ull);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) keep[n] = 0;
}

// the slot that holds `k`, claimed if no slot did; -1 when kVoxelProbeBound slots held other keys
__device__ __forceinline__ int64_t d_voxel_find_or_claim(VoxelSlot* table, const unsigned long long mask, const unsigned long long k) {
    unsigned long long idx = mix64(k) & mask;
#pragma unroll 1
    for (int probe = 0; probe < kVoxelProbeBound; ++probe) {
        unsigned long long prev = __hip_atomic_load(&table[idx].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == kEmpty) prev = atomicCAS(&table[idx].key, kEmpty, k);
        if (prev == kEmpty || prev == k) return (int64_t)idx;
        idx = (idx + 1) & mask;
    }
    return -1;
}

__global__ __launch_bounds__(kBlock) void k_voxel_claim(const int32_t* __restrict__ keep, const unsigned long long* __restrict__ key, const int64_t n,
                                                        const uint32_t scan_no, VoxelSlot* table, const unsigned long long mask, int32_t* __restrict__ slot_of,
                                                        unsigned long long* __restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int32_t slot = -1;
    if (keep[i]) {
        slot = (int32_t)d_voxel_find_or_claim(table, mask, key[i]);
        if (slot >= 0)
            atomicMin(&table[slot].owner, ((unsigned long long)scan_no << 32) | (unsigned long long)i);
        else
            atomicAdd(&counters[DC_PROBE_FAILED], 1ull);
    }
    slot_of[i] = slot;
}

__global__ __launch_bounds__(kBlock) void k_voxel_resolve(int32_t* __restrict__ keep, const int32_t* __restrict__ slot_of, const int64_t n, const uint32_t scan_no,
                                                          const VoxelSlot* __restrict__ table, unsigned long long* __restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const int32_t slot = slot_of[i];
    if (slot < 0) {  // (the call fails as a whole: DC_PROBE_FAILED)
        keep[i] = 0;
    } else if (table[slot].owner != (((unsigned long long)scan_no << 32) | (unsigned long long)i)) {
        keep[i] = 0;
        atomicAdd(&counters[DC_THINNED], 1ull);
    }
}

// A slot whose owner is a point of this scan was empty before the scan (an earlier scan's owner word is smaller and would have stayed), and
// no earlier key's probe sequence runs through it (it was empty when that key was entered): emptying these slots gives the table back
// exactly as it was.
__global__ __launch_bounds__(kBlock) void k_voxel_rollback(const int32_t* __restrict__ keep, const int32_t* __restrict__ slot_of, const int64_t n,
                                                           VoxelSlot* __restrict__ table) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const int32_t slot = slot_of[i];
    if (slot >= 0) table[slot].key = kEmpty, table[slot].owner = kEmpty;
}

__global__ __launch_bounds__(kBlock) void k_voxel_clear(VoxelSlot* __restrict__ table, const unsigned long long slots) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < slots) table[i].key = kEmpty, table[i].owner = kEmpty;
}

__global__ __launch_bounds__(kBlock) void k_voxel_rehash(const VoxelSlot* __restrict__ from, const unsigned long long from_slots, VoxelSlot* to,
                                                         const unsigned long long to_mask, unsigned long long* __restrict__ counters) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= from_slots) return;
    const VoxelSlot v = from[i];
    if (v.key == kEmpty) return;
    const int64_t slot = d_voxel_find_or_claim(to, to_mask, v.key);
    if (slot >= 0)
        atomicMin(&to[slot].owner, v.owner);
    else
        atomicAdd(&counters[DC_PROBE_FAILED], 1ull);
}

__global__ __launch_bounds__(kBlock) void k_dense_scatter(const float4* __restrict__ placed, const int32_t* __restrict__ keep, const int32_t* __restrict__ scan_excl,
                                                          const int64_t n, float4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n && keep[i]) out[scan_excl[i]] = placed[i];
}

// kFloats = 3: x y z; 4: x y z and the intensity of include/dmsa_dense_intensity.h, I7.  kLabel: one more word per row, the bits of the
// row's label (include/dmsa_dense_clusters.h, C7)
template <int kFloats, bool kLabel>
__global__ __launch_bounds__(kBlock) void k_dense_pack_rows(const float4* __restrict__ out, const int32_t* __restrict__ label, const int64_t m, float* __restrict__ rows) {
    constexpr int kWords = kFloats + (kLabel ? 1 : 0);
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // one word of the file per thread: coalesced stores
    if (j >= kWords * m) return;
    const int64_t k = j / kWords;
    const int a = (int)(j - kWords * k);
    if (kLabel && a == kFloats) {
        reinterpret_cast<int32_t*>(rows)[j] = label[k];
        return;
    }
    const float4 v = out[k];
    rows[j] = a == 0 ? v.x : a == 1 ? v.y : (kFloats == 3 || a == 2) ? v.z : v.w;
}

}  // namespace

void launch_dense_interpolate(DenseTraj tr, double max_pose_gap, const double* t, int64_t n, double* pose12, int32_t* segment, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_dense_interpolate, dim3(blocks_for(n)), dim3(kBlock), 0, s, tr, max_pose_gap, t, n, pose12, segment);
}
void launch_dense_place(const float4* xyz, const double* stamps, int64_t n, DenseTraj tr, DenseGates g, float4* placed, int32_t* keep, unsigned long long* key,
                        unsigned long long* counters, float4* origin, bool intensity, hipStream_t s) {
    if (n <= 0) return;
    if (intensity) hipLaunchKernelGGL(k_dense_place<true>, dim3(blocks_for(n)), dim3(kBlock), 0, s, xyz, stamps, n, tr, g, placed, keep, key, counters, origin);
    else hipLaunchKernelGGL(k_dense_place<false>, dim3(blocks_for(n)), dim3(kBlock), 0, s, xyz, stamps, n, tr, g, placed, keep, key, counters, origin);
}
void launch_voxel_claim(const int32_t* keep, const unsigned long long* key, int64_t n, uint32_t scan_no, VoxelSlot* table, uint64_t mask, int32_t* slot_of,
                        unsigned long long* counters, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_voxel_claim, dim3(blocks_for(n)), dim3(kBlock), 0, s, keep, key, n, scan_no, table, (unsigned long long)mask, slot_of, counters);
}
void launch_voxel_resolve(int32_t* keep, const int32_t* slot_of, int64_t n, uint32_t scan_no, const VoxelSlot* table, unsigned long long* counters, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_voxel_resolve, dim3(blocks_for(n)), dim3(kBlock), 0, s, keep, slot_of, n, scan_no, table, counters);
}
void launch_voxel_rollback(const int32_t* keep, const int32_t* slot_of, int64_t n, VoxelSlot* table, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_voxel_rollback, dim3(blocks_for(n)), dim3(kBlock), 0, s, keep, slot_of, n, table);
}
void launch_voxel_clear(VoxelSlot* table, uint64_t slots, hipStream_t s) {
    if (slots > 0) hipLaunchKernelGGL(k_voxel_clear, dim3(blocks_for(slots)), dim3(kBlock), 0, s, table, (unsigned long long)slots);
}
void launch_voxel_rehash(const VoxelSlot* from, uint64_t from_slots, VoxelSlot* to, uint64_t to_mask, unsigned long long* counters, hipStream_t s) {
    if (from_slots > 0)
        hipLaunchKernelGGL(k_voxel_rehash, dim3(blocks_for(from_slots)), dim3(kBlock), 0, s, from, (unsigned long long)from_slots, to, (unsigned long long)to_mask,
                           counters);
}
void launch_dense_scatter(const float4* placed, const int32_t* keep, const int32_t* scan_excl, int64_t n, float4* out, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_dense_scatter, dim3(blocks_for(n)), dim3(kBlock), 0, s, placed, keep, scan_excl, n, out);
}
void launch_dense_pack_rows(const float4* out, const int32_t* label, int64_t m, int row_floats, float* rows, hipStream_t s) {
    if (m <= 0) return;
    const dim3 grid(blocks_for((unsigned long long)(row_floats + (label ? 1 : 0)) * (unsigned long long)m));
    const auto kernel = label ? (row_floats == 4 ? k_dense_pack_rows<4, true> : k_dense_pack_rows<3, true>)
                              : (row_floats == 4 ? k_dense_pack_rows<4, false> : k_dense_pack_rows<3, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, out, label, m, rows);
}

}  // namespace dmsa
