// dense_normals.hip — the kernels of include/dmsa_dense_normals.h: a normal per point of the dense cloud from its radius neighbourhood.
//
//   k_normals_cell_keys / k_normals_count_cells / k_normals_cell_heads / k_normals_cell_ends   the search grid: cells of edge 1.001 * radius,
//                              the retained rows sorted by cell (the library's stable 64-bit sort: rows ascend inside a cell), a cell table
//   k_neighbour_moments        N2-N3, the hot kernel: ~100 candidates per query, ten exact int64 sums per query
//   k_normals_from_moments     N4, one thread per row (csrc/pcl_eigen33.h)
//   k_pack_normal_rows         the 28-byte rows of the file
//
// The grid is an implementation matter (N2): a neighbour is whatever passes the float distance test, and the grid only has to offer every such
// row as a candidate.  Its cells are cut in DOUBLE with an edge 0.1 % above the radius: a pair whose float d2 passes is at most
// radius * (1 + 2^-22) apart per axis, so its cells differ by at most one whatever the coordinates' size -- a float quotient would be off by up
// to 2^-4 cells at the far end of the 21-bit range.
//
// k_neighbour_moments: a WAVE owns 64 consecutive sorted rows, one query per lane.  It takes the box of its queries' cells grown by one cell,
// looks the box's cells up 64 at a time (a lane per cell), merges cells whose runs of sorted rows touch (cells that are neighbours along z do)
// and streams the runs in tiles of kNormalsTile rows: every lane loads one candidate, and the wave walks the tile with v_readlane, so a
// candidate costs the wave three scalar reads and no LDS.  Every lane tests every candidate of the box -- the d2 test is the definition, and a
// candidate two cells away fails it -- so each candidate is offered exactly once and the sums need no order: integer addition is
// associative.  Where 64 consecutive rows span a box of more than kNormalsBoxCells cells (the sorted order jumps between surfaces) the wave
// goes through its distinct cells one by one with the 27 cells around each, the other lanes masked.  One kernel shape serves a cell of 1 500
// rows (24 waves stream the same 27 cells) and 200 cells of one row (a wave packs 64 of them).  Built with -ffp-contract=off.
#include "dense_normals.h"

#include "pcl_eigen33.h"

#include <climits>
#include <cmath>

namespace dmsa {
namespace {

constexpr int kBlock = 256;
constexpr unsigned long long kEmptyKey = ~0ull;
constexpr int kCellBias = 1 << 20, kCellMax = (1 << 21) - 1;

inline unsigned blocks_for(unsigned long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

__device__ __forceinline__ unsigned long long d_mix64(unsigned long long x) {  // the finaliser of MurmurHash3, as the voxel table's
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}
__device__ __forceinline__ int d_cell_axis(const float v, const double cell) {
    const double c = floor((double)v / cell);
    const int b = (int)fmin(fmax(c, -1048576.0), 1048575.0) + kCellBias;  // (rule 6 and radius >= voxel_size keep c inside already)
    return b;
}
__device__ __forceinline__ unsigned long long d_cell_key(const int x, const int y, const int z) {
    return ((unsigned long long)x << 42) | ((unsigned long long)y << 21) | (unsigned long long)z;
}
// the slot of `key` in the table, or of the empty slot that ends its probe sequence (the table is at most half full)
__device__ __forceinline__ uint32_t d_cell_slot(const DenseCellEntry* table, const uint32_t mask, const unsigned long long key, bool* found) {
    uint32_t slot = (uint32_t)d_mix64(key) & mask;
    *found = false;
#pragma unroll 1
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const unsigned long long kk = table[slot].key;
        if (kk == key) {
            *found = true;
            return slot;
        }
        if (kk == kEmptyKey) return slot;
        slot = (slot + 1) & mask;
    }
    return slot;
}

__global__ __launch_bounds__(kBlock) void k_normals_cell_keys(const float4* __restrict__ g, const int64_t n, const double cell, unsigned long long* __restrict__ key,
                                                              uint32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 p = g[i];
    key[i] = d_cell_key(d_cell_axis(p.x, cell), d_cell_axis(p.y, cell), d_cell_axis(p.z, cell));
    idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_normals_count_cells(const unsigned long long* __restrict__ key, const int64_t n, unsigned long long* __restrict__ heads) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool head = i < n && (i == 0 || key[i - 1] != key[i]);
    const unsigned long long m = __ballot(head);
    if (m != 0ull && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(heads, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(kBlock) void k_normals_cell_heads(const float4* __restrict__ g, const uint32_t* __restrict__ idx, const unsigned long long* __restrict__ key,
                                                               const int64_t n, float4* __restrict__ pts, DenseCellEntry* table, const uint32_t mask) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    pts[i] = g[idx[i]];
    const unsigned long long k = key[i];
    if (i > 0 && key[i - 1] == k) return;
    uint32_t slot = (uint32_t)d_mix64(k) & mask;
#pragma unroll 1
    for (uint32_t probe = 0; probe <= mask; ++probe) {  // one insert per occupied cell: every key is entered once
        const unsigned long long prev = atomicCAS(&table[slot].key, kEmptyKey, k);
        if (prev == kEmptyKey) {
            table[slot].start = (uint32_t)i;
            return;
        }
        slot = (slot + 1) & mask;
    }
}

__global__ __launch_bounds__(kBlock) void k_normals_cell_ends(const unsigned long long* __restrict__ key, const int64_t n, DenseCellEntry* table, const uint32_t mask) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = key[i];
    if (i + 1 < n && key[i + 1] == k) return;
    bool found;
    const uint32_t slot = d_cell_slot(table, mask, k, &found);
    if (found) table[slot].end = (uint32_t)(i + 1);
}

__device__ __forceinline__ float d_lane_f(const float v, const int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ int d_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int d_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return __builtin_amdgcn_readfirstlane(v);
}

__global__ __launch_bounds__(kBlock) void k_neighbour_moments(const float4* __restrict__ pts, const uint32_t* __restrict__ idx, const unsigned long long* __restrict__ key,
                                                              const int64_t n, const DenseCellEntry* __restrict__ table, const uint32_t mask, const float r2,
                                                              const float scale, const int64_t first, const int64_t count, long long* __restrict__ moments) {
    const int lane = threadIdx.x & 63;
    const int64_t k = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 64 + lane;
    bool live = k < n;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    int64_t row = 0;
    unsigned long long my_key = kEmptyKey;
    if (live) {
        row = (int64_t)idx[k] - first;
        live = row >= 0 && row < count;
    }
    if (live) {
        const float4 p = pts[k];
        qx = p.x, qy = p.y, qz = p.z;
        my_key = key[k];
    }
    const unsigned long long act = __ballot(live);
    if (act == 0ull) return;  // (the whole wave: from here on every loop bound is the same in all 64 lanes)
    const int cx = (int)(my_key >> 42) & kCellMax, cy = (int)(my_key >> 21) & kCellMax, cz = (int)my_key & kCellMax;
    const int lox = d_wave_min(live ? cx : INT_MAX), loy = d_wave_min(live ? cy : INT_MAX), loz = d_wave_min(live ? cz : INT_MAX);
    const int hix = d_wave_max(live ? cx : INT_MIN), hiy = d_wave_max(live ? cy : INT_MIN), hiz = d_wave_max(live ? cz : INT_MIN);
    const bool whole = (unsigned long long)(hix - lox + 3) * (unsigned long long)(hiy - loy + 3) * (unsigned long long)(hiz - loz + 3) <=
                       (unsigned long long)kNormalsBoxCells;  // (each factor is at most 2^21 + 2: the product fits 64 bits)
    long long s_n = 0, s_x = 0, s_y = 0, s_z = 0, s_xx = 0, s_xy = 0, s_xz = 0, s_yy = 0, s_yz = 0, s_zz = 0;
    unsigned long long todo = act;
#pragma unroll 1
    while (todo != 0ull) {
        // this pass: a box of cells and the lanes whose queries it serves
        int bx, by, bz, ex, ey, ez;
        bool mine;
        if (whole) {
            bx = lox - 1, by = loy - 1, bz = loz - 1, ex = hix - lox + 3, ey = hiy - loy + 3, ez = hiz - loz + 3;
            mine = live, todo = 0ull;
        } else {
            const int leader = __ffsll((long long)todo) - 1;
            bx = __builtin_amdgcn_readlane(cx, leader) - 1, by = __builtin_amdgcn_readlane(cy, leader) - 1, bz = __builtin_amdgcn_readlane(cz, leader) - 1;
            ex = ey = ez = 3;
            mine = live && cx == bx + 1 && cy == by + 1 && cz == bz + 1;
            todo &= ~__ballot(mine);
        }
        const int cells = ex * ey * ez;
#pragma unroll 1
        for (int base = 0; base < cells; base += 64) {
            // a lane per cell of the box, z fastest: neighbours along z are neighbours in the sorted rows
            uint32_t cs = 0, ce = 0;
            const int c = base + lane;
            if (c < cells) {
                const int z = bz + c % ez, y = by + (c / ez) % ey, x = bx + c / (ez * ey);
                if (x >= 0 && x <= kCellMax && y >= 0 && y <= kCellMax && z >= 0 && z <= kCellMax) {
                    bool found;
                    const uint32_t slot = d_cell_slot(table, mask, d_cell_key(x, y, z), &found);
                    if (found) {
                        cs = table[slot].start, ce = table[slot].end;
                        if ((int64_t)ce > n) ce = (uint32_t)n;  // (never: every cell's end was entered)
                        if (cs > ce) cs = ce;
                    }
                }
            }
            unsigned long long has = __ballot(ce > cs);
            uint32_t rs = 0, re = 0;  // the run of sorted rows collected so far
#pragma unroll 1
            while (true) {
                const bool last = has == 0ull;
                uint32_t ns = 0, ne = 0;
                if (!last) {
                    const int l = __ffsll((long long)has) - 1;
                    has &= has - 1ull;
                    ns = (uint32_t)__builtin_amdgcn_readlane((int)cs, l), ne = (uint32_t)__builtin_amdgcn_readlane((int)ce, l);
                    if (re > rs && ns == re) {
                        re = ne;
                        continue;
                    }
                }
#pragma unroll 1
                for (uint32_t t = rs; t < re; t += kNormalsTile) {
                    const uint32_t j = t + (uint32_t)lane;
                    float4 cand = make_float4(INFINITY, INFINITY, INFINITY, 0.0f);  // (d2 = inf: never a neighbour)
                    if (j < re) cand = pts[j];
                    const int held = (int)min((uint32_t)kNormalsTile, re - t);
                    for (int u = 0; u < held; ++u) {
                        const float dx = d_lane_f(cand.x, u) - qx, dy = d_lane_f(cand.y, u) - qy, dz = d_lane_f(cand.z, u) - qz;
                        float d2 = dx * dx;
                        d2 += dy * dy;
                        d2 += dz * dz;
                        if (mine && d2 <= r2) {
                            const int ix = (int)rintf(dx * scale), iy = (int)rintf(dy * scale), iz = (int)rintf(dz * scale);
                            s_n += 1, s_x += ix, s_y += iy, s_z += iz;
                            s_xx += (long long)ix * ix, s_xy += (long long)ix * iy, s_xz += (long long)ix * iz;
                            s_yy += (long long)iy * iy, s_yz += (long long)iy * iz, s_zz += (long long)iz * iz;
                        }
                    }
                }
                if (last) break;
                rs = ns, re = ne;
            }
        }
    }
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

__global__ __launch_bounds__(kBlock) void k_pack_normal_rows(const float4* __restrict__ g, const float4* __restrict__ normal, const int64_t first, const int64_t m,
                                                             float* __restrict__ rows) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // one float of the file per thread: coalesced stores
    if (j >= 7 * m) return;
    const int64_t k = j / 7;
    const int a = (int)(j - 7 * k);
    const float4 v = a < 3 ? g[first + k] : normal[first + k];
    const int b = a < 3 ? a : a - 3;
    rows[j] = b == 0 ? v.x : b == 1 ? v.y : b == 2 ? v.z : v.w;
}

}  // namespace

void launch_normals_cell_keys(const float4* g, int64_t n, double cell, unsigned long long* key, uint32_t* idx, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_normals_cell_keys, dim3(blocks_for(n)), dim3(kBlock), 0, s, g, n, cell, key, idx);
}
void launch_normals_count_cells(const unsigned long long* key_sorted, int64_t n, unsigned long long* heads, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_normals_count_cells, dim3(blocks_for(n)), dim3(kBlock), 0, s, key_sorted, n, heads);
}
void launch_normals_cell_heads(const float4* g, const uint32_t* idx_sorted, const unsigned long long* key_sorted, int64_t n, float4* pts_sorted,
                               DenseCellEntry* table, uint32_t mask, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_normals_cell_heads, dim3(blocks_for(n)), dim3(kBlock), 0, s, g, idx_sorted, key_sorted, n, pts_sorted, table, mask);
}
void launch_normals_cell_ends(const unsigned long long* key_sorted, int64_t n, DenseCellEntry* table, uint32_t mask, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_normals_cell_ends, dim3(blocks_for(n)), dim3(kBlock), 0, s, key_sorted, n, table, mask);
}
void launch_neighbour_moments(const float4* pts_sorted, const uint32_t* idx_sorted, const unsigned long long* key_sorted, int64_t n, const DenseCellEntry* table,
                              uint32_t mask, float r2, float scale, int64_t first, int64_t count, long long* moments, hipStream_t s) {
    if (n > 0 && count > 0)
        hipLaunchKernelGGL(k_neighbour_moments, dim3(blocks_for(n)), dim3(kBlock), 0, s, pts_sorted, idx_sorted, key_sorted, n, table, mask, r2, scale, first, count,
                           moments);
}
void launch_normals_from_moments(const long long* moments, const float4* g, const float4* origin, int64_t first, int64_t count, int32_t min_neighbours,
                                 float4* normal, unsigned long long* without, hipStream_t s) {
    if (count > 0)
        hipLaunchKernelGGL(k_normals_from_moments, dim3(blocks_for(count)), dim3(kBlock), 0, s, moments, g, origin, first, count, min_neighbours, normal, without);
}
void launch_pack_normal_rows(const float4* g, const float4* normal, int64_t first, int64_t m, float* rows, hipStream_t s) {
    if (m > 0) hipLaunchKernelGGL(k_pack_normal_rows, dim3(blocks_for(7 * (unsigned long long)m)), dim3(kBlock), 0, s, g, normal, first, m, rows);
}

}  // namespace dmsa
