// dense_normals.hip — the kernels of include/dmsa_dense_normals.h: a normal per point of the dense cloud from its radius neighbourhood.
//
//   k_neighbour_moments        N2-N3, the hot kernel: ~100 candidates per query, ten exact int64 sums per query
//   k_normals_from_moments     N4, one thread per row (csrc/pcl_eigen33.h)
//   k_pack_normal_rows         the 28-byte rows of the file (32-byte rows with an intensity)
//
// k_neighbour_moments: the traversal of csrc/dense_grid_walk.h over the search grid of csrc/dense_grid.hip (a wave owns 64 consecutive sorted rows and streams the box of their cells once, in
// register tiles walked with v_readlane) with the ten sums as its per-candidate step.  Each candidate is offered exactly once and the sums
// need no order: integer addition is associative.  One kernel shape serves a cell of 1 500 rows (24 waves stream the same 27 cells) and
// 200 cells of one row (a wave packs 64 of them).  Built with -ffp-contract=off.
#include "dense_normals.h"

#include "dense_grid_walk.h"
#include "pcl_eigen33.h"

#include <cmath>

namespace dmsa {
namespace {

__global__ __launch_bounds__(kBlock) void k_neighbour_moments(const float4* __restrict__ pts, const uint32_t* __restrict__ idx, const unsigned long long* __restrict__ key,
                                                              const int64_t n, const DenseCellEntry* __restrict__ table, const uint32_t mask, const float r2,
                                                              const float scale, const int64_t first, const int64_t count, long long* __restrict__ moments) {
    const int lane = threadIdx.x & 63;
    const int64_t k = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 64 + lane;
    bool live = k < n;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    int64_t row = 0;
    unsigned long long my_key = kCellEmptyKey;
    if (live) {
        row = (int64_t)idx[k] - first;
        live = row >= 0 && row < count;
    }
    if (live) {
        const float4 p = pts[k];
        qx = p.x, qy = p.y, qz = p.z;
        my_key = key[k];
    }
    if (__ballot(live) == 0ull) return;  // (the whole wave)
    long long s_n = 0, s_x = 0, s_y = 0, s_z = 0, s_xx = 0, s_xy = 0, s_xz = 0, s_yy = 0, s_yz = 0, s_zz = 0;
    d_walk_candidates(pts, n, table, mask, lane, live, my_key, [&](const bool mine, const float x, const float y, const float z, const uint32_t) {
        const float dx = x - qx, dy = y - qy, dz = z - qz;
        float d2 = dx * dx;
        d2 += dy * dy;
        d2 += dz * dz;
        if (mine && d2 <= r2) {
            const int ix = (int)rintf(dx * scale), iy = (int)rintf(dy * scale), iz = (int)rintf(dz * scale);
            s_n += 1, s_x += ix, s_y += iy, s_z += iz;
            s_xx += (long long)ix * ix, s_xy += (long long)ix * iy, s_xz += (long long)ix * iz;
            s_yy += (long long)iy * iy, s_yz += (long long)iy * iz, s_zz += (long long)iz * iz;
        }
    });
    if (live) {
        long long* m = moments + row * 10;
        m[0] = s_n, m[1] = s_x, m[2] = s_y, m[3] = s_z, m[4] = s_xx, m[5] = s_xy, m[6] = s_xz, m[7] = s_yy, m[8] = s_yz, m[9] = s_zz;
    }
}

__global__ __launch_bounds__(kBlock) void k_normals_from_moments(const long long* __restrict__ moments, const float4* __restrict__ g, const float4* __restrict__ origin,
                                                                 const int64_t first, const int64_t count, const int32_t min_neighbours, float4* __restrict__ normal,
                                                                 unsigned long long* __restrict__ without) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool none = false;
    if (i < count) {
        long long m[10];
#pragma unroll
        for (int a = 0; a < 10; ++a) m[a] = moments[i * 10 + a];
        const float4 p = g[first + i], o = origin[first + i];
        float out[4];
        none = !dense_normal_from_moments(m, o.x - p.x, o.y - p.y, o.z - p.z, min_neighbours, out);
        normal[first + i] = make_float4(out[0], out[1], out[2], out[3]);
    }
    const unsigned long long b = __ballot(none);
    if (b != 0ull && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)b) - 1)) atomicAdd(without, (unsigned long long)__popcll(b));
}

// kFloats = 7: x y z and the normal; 8: x y z, the intensity of include/dmsa_dense_intensity.h (I7) and the normal
template <int kFloats>
__global__ __launch_bounds__(kBlock) void k_pack_normal_rows(const float4* __restrict__ g, const float4* __restrict__ normal, const int64_t first, const int64_t m,
                                                             float* __restrict__ rows) {
    constexpr int kOwn = kFloats - 4;                              // floats of the row that come from the point
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // one float of the file per thread: coalesced stores
    if (j >= kFloats * m) return;
    const int64_t k = j / kFloats;
    const int a = (int)(j - kFloats * k);
    const float4 v = a < kOwn ? g[first + k] : normal[first + k];
    const int b = a < kOwn ? a : a - kOwn;
    rows[j] = b == 0 ? v.x : b == 1 ? v.y : b == 2 ? v.z : v.w;
}

}  // namespace

void launch_neighbour_moments(const GridView& grid, float r2, float scale, int64_t first, int64_t count, long long* moments, hipStream_t s) {
    if (grid.n > 0 && count > 0)
        hipLaunchKernelGGL(k_neighbour_moments, dim3(blocks_for(grid.n)), dim3(kBlock), 0, s, grid.pts_sorted, grid.idx_sorted, grid.key_sorted, grid.n, grid.table,
                           grid.mask, r2, scale, first, count, moments);
}
void launch_normals_from_moments(const long long* moments, const float4* g, const float4* origin, int64_t first, int64_t count, int32_t min_neighbours,
                                 float4* normal, unsigned long long* without, hipStream_t s) {
    if (count > 0)
        hipLaunchKernelGGL(k_normals_from_moments, dim3(blocks_for(count)), dim3(kBlock), 0, s, moments, g, origin, first, count, min_neighbours, normal, without);
}
void launch_pack_normal_rows(const float4* g, const float4* normal, int64_t first, int64_t m, int row_floats, float* rows, hipStream_t s) {
    if (m <= 0) return;
    const dim3 grid(blocks_for((unsigned long long)row_floats * (unsigned long long)m));
    if (row_floats == 8) hipLaunchKernelGGL(k_pack_normal_rows<8>, grid, dim3(kBlock), 0, s, g, normal, first, m, rows);
    else hipLaunchKernelGGL(k_pack_normal_rows<7>, grid, dim3(kBlock), 0, s, g, normal, first, m, rows);
}

}  // namespace dmsa
