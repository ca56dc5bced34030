// dense_occupancy.h — launchers of the kernels behind include/dmsa_dense_occupancy.h (csrc/dense_occupancy.hip): every retained ray walked
// with csrc/dense_carve_walk.h into a table of {cell key, hits, passes} (M2-M3), the table's cells listed in key order with their states
// (M4-M5), the rows of the voxel file (M6) and the slice (M7).  Scan and sort are the library's own (device_prims.h).
#pragma once
#include "dense_grid.h"

namespace dmsa {

// the table of M3: DenseCellEntry's scheme (open addressing, linear probing, an all-ones key = empty) with the two counters in its two words
struct OccupancySlot {
    unsigned long long key;  // three biased 21-bit cells, as d_cell_key builds it
    uint32_t hits, passes;
};
// the scalars of dmsa_dense_occupancy_config the kernels read
struct OccupancyParams {
    double cell;  // (double)cell_size
    float max_length;
    uint32_t min_hits, min_passes, occ_num, occ_den;
};
// the record of a walk in HBM, zeroed before k_occupancy_walk: the one small read of a build
enum OccupancyWord { OW_OVERFLOW = 0, OW_OCCUPIED, OW_SKIPPED, OW_CELLS, OW_OUT_OF_RANGE, OW_COUNT };
// the sums of the listing (the three states) and of a slice (the slab's cells, the three pixel values)
enum OccupancySum { OS_UNKNOWN = 0, OS_FREE, OS_OCCUPIED, OS_STATES };
// the extents of a slice: int32 words, set to INT_MAX / INT_MIN by the launcher's caller through launch_occupancy_extent_init
enum OccupancyExtent { OE_X_MIN = 0, OE_Y_MIN, OE_X_MAX, OE_Y_MAX, OE_COUNT };

// every slot empty with both counters 0
void launch_occupancy_clear(OccupancySlot* table, uint64_t slots, hipStream_t s);
// M2-M3 for all rows of the grid, a ray per lane in sorted order; rec[OW_*] += this launch's share.  A table with more than `limit` keys, or a
// probe that runs out of slots, sets rec[OW_OVERFLOW]: the counts are then incomplete and the caller walks again into a larger table.
void launch_occupancy_walk(const GridView& grid, const float4* origin, OccupancyParams p, OccupancySlot* table, uint32_t mask, uint64_t limit,
                           unsigned long long* rec, hipStream_t s);
// flag[i] = slot i holds a key, for i < slots; flag[slots] = 0
void launch_occupancy_flags(const OccupancySlot* table, uint64_t slots, int32_t* flag, hipStream_t s);
// key[scan[i]] = slot i's key, slot_of[scan[i]] = i for every slot that holds one (m of them: the room in key and slot_of)
void launch_occupancy_compact(const OccupancySlot* table, uint64_t slots, const int32_t* flag, const int32_t* scan, int64_t m, unsigned long long* key, uint32_t* slot_of,
                              hipStream_t s);
// per listed cell j (m of them, slot_sorted[j] its slot): hits, passes, M5's state; sums[OS_*] += cells of each state
void launch_occupancy_states(const OccupancySlot* table, const uint32_t* slot_sorted, int64_t m, OccupancyParams p, uint32_t* hits, uint32_t* passes, uint32_t* state,
                             unsigned long long* sums, hipStream_t s);
// keep[j] = state[j] >= min_state for j < m; keep[m] = 0
void launch_occupancy_select_flags(const uint32_t* state, int64_t m, uint32_t min_state, int32_t* keep, hipStream_t s);
// sel[scan[j]] = j for every kept cell
void launch_occupancy_select(const int32_t* keep, const int32_t* scan, int64_t m, uint32_t* sel, hipStream_t s);
// M6: `count` rows of 24 bytes for the listed cells sel[first .. first + count) (sel null: the cells first .. first + count themselves)
void launch_occupancy_rows(const unsigned long long* key, const uint32_t* hits, const uint32_t* passes, const uint32_t* state, const uint32_t* sel, int64_t first,
                           int64_t count, double cell, uint32_t* out, hipStream_t s);
// M7: extent[OE_*] = the bounding box of the columns of the slab cz_lo <= cz <= cz_hi (biased cells; extent preset by the _init launcher)
void launch_occupancy_extent_init(int32_t* extent, hipStream_t s);
void launch_occupancy_extent(const unsigned long long* key, int64_t m, int32_t cz_lo, int32_t cz_hi, int32_t* extent, hipStream_t s);
// image[(y_max - cy) * width + cx - x_min] |= 1 << state for every listed cell of the slab (image zeroed by the caller; biased cells)
void launch_occupancy_columns(const unsigned long long* key, const uint32_t* state, int64_t m, int32_t cz_lo, int32_t cz_hi, int32_t x_min, int32_t y_max, int32_t width,
                              int32_t height, uint32_t* image, hipStream_t s);
// pixels[i] = 0 / 254 / 205 from image[i]'s bits; sums[OS_*] += pixels of each value
void launch_occupancy_pixels(const uint32_t* image, int64_t n, uint8_t* pixels, unsigned long long* sums, hipStream_t s);

}  // namespace dmsa
