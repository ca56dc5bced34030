// dense_grid.hip — the kernels that build the search grid over the retained rows of a dense cloud (csrc/dense_grid.h), for the normals, the
// outlier classification and the ray carving alike.
//
//   k_grid_cell_keys / k_grid_count_cells / k_grid_cell_heads / k_grid_cell_ends   cells of the edge asked for, the retained rows sorted by
//                              cell (the library's stable 64-bit sort: rows ascend inside a cell), a cell table
//
// The grid is an implementation matter (N2): a neighbour is whatever passes the float distance test, and the grid only has to offer every such
// row as a candidate.  Its cells are cut in DOUBLE; the neighbourhood calls ask for an edge 0.1 % above the radius: a pair whose float d2
// passes is at most radius * (1 + 2^-22) apart per axis, so its cells differ by at most one whatever the coordinates' size -- a float quotient
// would be off by up to 2^-4 cells at the far end of the 21-bit range.  Built with -ffp-contract=off.
#include "dense_grid.h"

#include "dense_dev.h"
#include "dense_grid_walk.h"

#include <cmath>

namespace dmsa {
namespace {

__device__ __forceinline__ int d_cell_axis(const float v, const double cell) {
    const double c = floor((double)v / cell);
    const int b = (int)fmin(fmax(c, -1048576.0), 1048575.0) + kCellBias;  // (rule 6 and radius >= voxel_size keep c inside already)
    return b;
}
__global__ __launch_bounds__(kBlock) void k_grid_cell_keys(const float4* __restrict__ g, const int64_t n, const double cell, unsigned long long* __restrict__ key,
                                                           uint32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 p = g[i];
    key[i] = d_cell_key(d_cell_axis(p.x, cell), d_cell_axis(p.y, cell), d_cell_axis(p.z, cell));
    idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_grid_count_cells(const unsigned long long* __restrict__ key, const int64_t n, unsigned long long* __restrict__ heads) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool head = i < n && (i == 0 || key[i - 1] != key[i]);
    const unsigned long long m = __ballot(head);
    if (m != 0ull && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(heads, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(kBlock) void k_grid_cell_heads(const float4* __restrict__ g, const uint32_t* __restrict__ idx, const unsigned long long* __restrict__ key,
                                                            const int64_t n, float4* __restrict__ pts, DenseCellEntry* table, const uint32_t mask) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    pts[i] = g[idx[i]];
    const unsigned long long k = key[i];
    if (i > 0 && key[i - 1] == k) return;
    uint32_t slot = (uint32_t)mix64(k) & mask;
#pragma unroll 1
    for (uint32_t probe = 0; probe <= mask; ++probe) {  // one insert per occupied cell: every key is entered once
        const unsigned long long prev = atomicCAS(&table[slot].key, kCellEmptyKey, k);
        if (prev == kCellEmptyKey) {
            table[slot].start = (uint32_t)i;
            return;
        }
        slot = (slot + 1) & mask;
    }
}

__global__ __launch_bounds__(kBlock) void k_grid_cell_ends(const unsigned long long* __restrict__ key, const int64_t n, DenseCellEntry* table, const uint32_t mask) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = key[i];
    if (i + 1 < n && key[i + 1] == k) return;
    bool found;
    const uint32_t slot = d_cell_slot(table, mask, k, &found);
    if (found) table[slot].end = (uint32_t)(i + 1);
}

}  // namespace

void launch_grid_cell_keys(const float4* g, int64_t n, double cell, unsigned long long* key, uint32_t* idx, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_grid_cell_keys, dim3(blocks_for(n)), dim3(kBlock), 0, s, g, n, cell, key, idx);
}
void launch_grid_count_cells(const unsigned long long* key_sorted, int64_t n, unsigned long long* heads, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_grid_count_cells, dim3(blocks_for(n)), dim3(kBlock), 0, s, key_sorted, n, heads);
}
void launch_grid_cell_heads(const float4* g, const uint32_t* idx_sorted, const unsigned long long* key_sorted, int64_t n, float4* pts_sorted, DenseCellEntry* table,
                            uint32_t mask, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_grid_cell_heads, dim3(blocks_for(n)), dim3(kBlock), 0, s, g, idx_sorted, key_sorted, n, pts_sorted, table, mask);
}
void launch_grid_cell_ends(const unsigned long long* key_sorted, int64_t n, DenseCellEntry* table, uint32_t mask, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_grid_cell_ends, dim3(blocks_for(n)), dim3(kBlock), 0, s, key_sorted, n, table, mask);
}

}  // namespace dmsa
