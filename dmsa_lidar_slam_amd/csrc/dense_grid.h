// dense_grid.h — the search grid over the retained rows of a dense cloud (csrc/dense_grid.hip): its cell table, the view the walking kernels
// of the three stages take, and the launchers of the four kernels that build it.
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
// a built grid as the stages' launchers take it (the kernels take its members one by one)
struct GridView {
    const float4* pts_sorted;
    const uint32_t* idx_sorted;
    const unsigned long long* key_sorted;
    int64_t n;
    const DenseCellEntry* table;
    uint32_t mask;
};
constexpr int kGridTile = 64;       // candidates a wave of d_walk_candidates holds in registers at a time (one per lane)
constexpr int kGridBoxCells = 512;  // cells of the box around a wave's queries up to which the wave streams the box once for all its lanes

// key[i] = cell of g[i] (edge `cell`, computed in double, biased by 2^20, x << 42 | y << 21 | z), idx[i] = i
void launch_grid_cell_keys(const float4* g, int64_t n, double cell, unsigned long long* key, uint32_t* idx, hipStream_t s);
// *heads += sorted rows whose key differs from the row before (= occupied cells)
void launch_grid_count_cells(const unsigned long long* key_sorted, int64_t n, unsigned long long* heads, hipStream_t s);
// pts_sorted[k] = g[idx_sorted[k]]; the first row of every cell enters the cell's key and `start` into the table (cleared to 0xFF) ...
void launch_grid_cell_heads(const float4* g, const uint32_t* idx_sorted, const unsigned long long* key_sorted, int64_t n, float4* pts_sorted,
                            DenseCellEntry* table, uint32_t mask, hipStream_t s);
// ... and, in a launch of its own, the last row of every cell its `end`
void launch_grid_cell_ends(const unsigned long long* key_sorted, int64_t n, DenseCellEntry* table, uint32_t mask, hipStream_t s);

}  // namespace dmsa
