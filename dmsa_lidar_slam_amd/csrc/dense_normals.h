// dense_normals.h — launchers of the kernels behind include/dmsa_dense_normals.h (csrc/dense_normals.hip): the search grid over the retained
// points, the exact integer moments of every radius neighbourhood, the normals and the 28-byte rows of their file.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dmsa {

// the cell table: the CellHashEntry scheme of static_kernels.h (open addressing, linear probing, ~0 = empty) with the end of the cell's run
// of sorted rows in the word that is padding there
struct DenseCellEntry {
    unsigned long long key;  // three biased 21-bit cells
    uint32_t start, end;     // sorted rows [start, end) lie in the cell
};
constexpr int kNormalsTile = 64;       // candidates a wave of k_neighbour_moments holds in registers at a time (one per lane)
constexpr int kNormalsBoxCells = 512;  // cells of the box around a wave's queries up to which the wave streams the box once for all its lanes

// key[i] = cell of g[i] (edge `cell`, computed in double, biased by 2^20, x << 42 | y << 21 | z), idx[i] = i
void launch_normals_cell_keys(const float4* g, int64_t n, double cell, unsigned long long* key, uint32_t* idx, hipStream_t s);
// *heads += sorted rows whose key differs from the row before (= occupied cells)
void launch_normals_count_cells(const unsigned long long* key_sorted, int64_t n, unsigned long long* heads, hipStream_t s);
// pts_sorted[k] = g[idx_sorted[k]]; the first row of every cell enters the cell's key and `start` into the table (cleared to 0xFF) ...
void launch_normals_cell_heads(const float4* g, const uint32_t* idx_sorted, const unsigned long long* key_sorted, int64_t n, float4* pts_sorted,
                               DenseCellEntry* table, uint32_t mask, hipStream_t s);
// ... and, in a launch of its own, the last row of every cell its `end`
void launch_normals_cell_ends(const unsigned long long* key_sorted, int64_t n, DenseCellEntry* table, uint32_t mask, hipStream_t s);
// N2-N3 for the retained rows [first, first + count): moments[(row - first) * 10 + 0..9]
void launch_neighbour_moments(const float4* pts_sorted, const uint32_t* idx_sorted, const unsigned long long* key_sorted, int64_t n, const DenseCellEntry* table,
                              uint32_t mask, float r2, float scale, int64_t first, int64_t count, long long* moments, hipStream_t s);
// N4 for rows [first, first + count): normal[first + i] from moments[10 i ..]; *without += rows that got NaNs
void launch_normals_from_moments(const long long* moments, const float4* g, const float4* origin, int64_t first, int64_t count, int32_t min_neighbours,
                                 float4* normal, unsigned long long* without, hipStream_t s);
// rows[7 k .. 7 k + 6] = g[first + k].xyz, normal[first + k] (nx, ny, nz, curvature)
void launch_pack_normal_rows(const float4* g, const float4* normal, int64_t first, int64_t m, float* rows, hipStream_t s);

}  // namespace dmsa
