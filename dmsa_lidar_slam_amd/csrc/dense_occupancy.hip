// dense_occupancy.hip — the kernels of include/dmsa_dense_occupancy.h: the occupancy map of the dense cloud from its measured rays.
//
//   k_occupancy_clear          every slot of the table empty, both counters 0
//   k_occupancy_walk           M2-M3, the hot kernel: one ray per lane, walked with csrc/dense_carve_walk.h into the table
//   k_occupancy_flags          a flag per slot that holds a key (scanned by the library's exclusive scan)
//   k_occupancy_compact        keys and slot numbers of the held slots, side by side (sorted by the library's 64-bit sort: M4)
//   k_occupancy_states         hits, passes and M5's state per listed cell, and the cells of each state
//   k_occupancy_select_flags   M6: state >= min_state per listed cell; k_occupancy_select: the listed cells that pass, in order
//   k_occupancy_rows           M6: the 24-byte rows of a chunk of the voxel file
//   k_occupancy_extent         M7: the bounding box of the slab's columns (wave reductions, then atomicMin / atomicMax)
//   k_occupancy_columns        M7: one thread per listed cell ORs its state's bit into the image word of its column
//   k_occupancy_pixels         M7: one thread per pixel: 0 / 254 / 205, and the pixels of each value
//
// k_occupancy_walk takes its rays in the grid's SORTED row order, for the reason stated at the top of dense_carve.hip: the 64 rays of a wave
// leave from nearly one origin and end in the same few cells.  Near the sensor all of them stand in the same cell in the same step, so before
// any atomic the wave MERGES: a leader's (key, counter) tag is broadcast, __ballot collects the lanes with the same tag, the leader keeps the
// popcount, and the round repeats over the lanes left (at most 64 rounds, registers and scalar moves only).  Then every leader, all at once,
// finds or inserts its key (DenseCellEntry's scheme: a 64-bit atomicCAS on the key, linear probing, an all-ones key is empty) and adds its
// count with ONE 32-bit vector atomicAdd.  Hits and passes of one cell in one step are two tags: the counters stay apart.
// Every loop has a bound: the walk kCarveMaxSteps, the merge 64, the probe the slot count.  Nothing waits for another lane.  A table with
// more keys than `limit`, or a probe that runs out, sets rec[OW_OVERFLOW]; the wave stops, and the host walks again into a larger table.
// Integer sums throughout: the result does not depend on lane, wave or atomic order.  No LDS.  Built with -ffp-contract=off.
#include "dense_occupancy.h"

#include "dense_grid_walk.h"
#include "dense_occupancy_rule.h"

namespace dmsa {
namespace {

constexpr int kAgentRelaxed = __ATOMIC_RELAXED;

__global__ __launch_bounds__(kBlock) void k_occupancy_clear(OccupancySlot* __restrict__ table, const unsigned long long slots) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < slots) reinterpret_cast<uint4*>(table)[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
}

// the slot that holds `key`, entered if no slot did (*inserted); -1 when every slot held another key
__device__ __forceinline__ int64_t d_occupancy_find_or_insert(OccupancySlot* table, const uint32_t mask, const unsigned long long key, bool* inserted) {
    uint32_t slot = (uint32_t)mix64(key) & mask;
#pragma unroll 1
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        unsigned long long prev = __hip_atomic_load(&table[slot].key, kAgentRelaxed, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == kCellEmptyKey) {
            prev = atomicCAS(&table[slot].key, kCellEmptyKey, key);
            if (prev == kCellEmptyKey) {
                *inserted = true;
                return (int64_t)slot;
            }
        }
        if (prev == key) return (int64_t)slot;
        slot = (slot + 1) & mask;
    }
    return -1;
}

__global__ __launch_bounds__(kBlock) void k_occupancy_walk(const float4* __restrict__ pts, const uint32_t* __restrict__ idx, const float4* __restrict__ origin,
                                                           const int64_t n, const OccupancyParams p, OccupancySlot* table, const uint32_t mask,
                                                           const unsigned long long limit, unsigned long long* rec) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t self = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // this lane's sorted row: its ray
    // a wave that starts after the table overflowed has nothing to add: the host walks again
    if (__ballot(__hip_atomic_load(rec + OW_OVERFLOW, kAgentRelaxed, __HIP_MEMORY_SCOPE_AGENT) != 0ull) != 0ull) return;
    unsigned long long skipped = 0ull, cells = 0ull, outside = 0ull;
    CarveWalk w{};
    bool active = false;
    if (self < n) {
        const float4 g = pts[self], o = origin[idx[self]];
        const CarveRay ray = carve_ray(o.x, o.y, o.z, g.x, g.y, g.z);
        if (carve_ray_skipped(ray, p.max_length) || !carve_walk_begin(p.cell, o.x, o.y, o.z, g.x, g.y, g.z, &w)) skipped = 1ull;
        else active = true;
    }
#pragma unroll 1
    for (int32_t step = 0; step <= kCarveMaxSteps; ++step) {  // (T4: every lane's walk ends before the bound does)
        if (__ballot(active) == 0ull) break;
        const bool inside = active && carve_cell_holds_rows(w);
        // M3: the walk stands in its last cell iff no plane is left to cross
        const unsigned long long last = (w.lx > 0 || w.ly > 0 || w.lz > 0) ? 0ull : 1ull;
        const unsigned long long tag = inside ? (d_cell_key(w.cx + kCellBias, w.cy + kCellBias, w.cz + kCellBias) << 1) | last : 0ull;
        // the merge: `mine` = lanes of this step with this lane's tag, in the first of them; 0 in the others
        uint32_t mine = 0u;
        unsigned long long todo = __ballot(inside);
#pragma unroll 1
        for (int round = 0; round < 64 && todo != 0ull; ++round) {
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned long long lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)tag, leader);
            const unsigned long long hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(tag >> 32), leader);
            const unsigned long long group = __ballot(inside && tag == ((hi << 32) | lo));
            if (lane == leader) mine = (uint32_t)__popcll(group);
            todo &= ~group & ~(1ull << leader);  // (the leader is in its own group: every round takes at least one lane)
        }
        bool inserted = false, gave_up = false;
        if (mine != 0u) {
            const int64_t slot = d_occupancy_find_or_insert(table, mask, tag >> 1, &inserted);
            if (slot < 0) gave_up = true;
            else atomicAdd((tag & 1ull) ? &table[slot].hits : &table[slot].passes, mine);
        }
        // the keys in the table, counted once per wave and step; past `limit` the table is too full to go on
        const unsigned long long entered = __ballot(inserted);
        if (entered != 0ull && lane == __ffsll((long long)entered) - 1) {
            const unsigned long long now = (unsigned long long)__popcll(entered);
            if (atomicAdd(rec + OW_OCCUPIED, now) + now > limit) gave_up = true;
        }
        if (__ballot(gave_up) != 0ull) {
            if (gave_up) atomicMax(rec + OW_OVERFLOW, 1ull);
            break;  // the whole wave: this walk's counts are discarded
        }
        if (active) {
            ++cells;
            if (!inside) ++outside;
            if (!carve_walk_step(&w)) active = false;
        }
    }
    skipped = wave_sum(skipped), cells = wave_sum(cells), outside = wave_sum(outside);
    if (lane == 0) {
        if (skipped != 0ull) atomicAdd(rec + OW_SKIPPED, skipped);
        if (cells != 0ull) atomicAdd(rec + OW_CELLS, cells);
        if (outside != 0ull) atomicAdd(rec + OW_OUT_OF_RANGE, outside);
    }
}

__global__ __launch_bounds__(kBlock) void k_occupancy_flags(const OccupancySlot* __restrict__ table, const unsigned long long slots, int32_t* __restrict__ flag) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i > slots) return;
    flag[i] = i < slots && table[i].key != kCellEmptyKey ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void k_occupancy_compact(const OccupancySlot* __restrict__ table, const unsigned long long slots, const int32_t* __restrict__ flag,
                                                              const int32_t* __restrict__ scan, const int64_t m, unsigned long long* __restrict__ key,
                                                              uint32_t* __restrict__ slot_of) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= slots || flag[i] == 0) return;
    const int64_t at = (int64_t)scan[i];
    if (at < 0 || at >= m) return;  // (never: the walk counted the keys it entered)
    key[at] = table[i].key, slot_of[at] = (uint32_t)i;
}

// sums[which] += lanes of the wave with `yes`, one atomic per wave and sum
__device__ __forceinline__ void d_count_lanes(const bool yes, unsigned long long* sum) {
    const unsigned long long m = __ballot(yes);
    if (m != 0ull && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(sum, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(kBlock) void k_occupancy_states(const OccupancySlot* __restrict__ table, const uint32_t* __restrict__ slot_sorted, const int64_t m,
                                                             const OccupancyParams p, uint32_t* __restrict__ hits, uint32_t* __restrict__ passes,
                                                             uint32_t* __restrict__ state, unsigned long long* __restrict__ sums) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t s = 0xFFFFFFFFu;
    if (j < m) {
        const OccupancySlot e = table[slot_sorted[j]];
        s = occupancy_state(p.min_hits, p.min_passes, p.occ_num, p.occ_den, e.hits, e.passes);
        hits[j] = e.hits, passes[j] = e.passes, state[j] = s;
    }
    d_count_lanes(s == kOccupancyUnknown, sums + OS_UNKNOWN);
    d_count_lanes(s == kOccupancyFree, sums + OS_FREE);
    d_count_lanes(s == kOccupancyOccupied, sums + OS_OCCUPIED);
}

__global__ __launch_bounds__(kBlock) void k_occupancy_select_flags(const uint32_t* __restrict__ state, const int64_t m, const uint32_t min_state, int32_t* __restrict__ keep) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j > m) return;
    keep[j] = j < m && state[j] >= min_state ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void k_occupancy_select(const int32_t* __restrict__ keep, const int32_t* __restrict__ scan, const int64_t m, uint32_t* __restrict__ sel) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= m || keep[j] == 0) return;
    const int64_t at = (int64_t)scan[j];
    if (at >= 0 && at < m) sel[at] = (uint32_t)j;  // (always: at <= j)
}

__device__ __forceinline__ int d_key_x(const unsigned long long key) { return (int)(key >> 42) & kCellMax; }
__device__ __forceinline__ int d_key_y(const unsigned long long key) { return (int)(key >> 21) & kCellMax; }
__device__ __forceinline__ int d_key_z(const unsigned long long key) { return (int)key & kCellMax; }

__global__ __launch_bounds__(kBlock) void k_occupancy_rows(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ hits, const uint32_t* __restrict__ passes,
                                                           const uint32_t* __restrict__ state, const uint32_t* __restrict__ sel, const int64_t first, const int64_t count,
                                                           const double cell, uint32_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= count) return;
    const int64_t j = sel ? (int64_t)sel[first + t] : first + t;
    const unsigned long long k = key[j];
    uint32_t* row = out + 6 * t;
    row[0] = __float_as_uint(occupancy_centre(d_key_x(k) - kCellBias, cell));
    row[1] = __float_as_uint(occupancy_centre(d_key_y(k) - kCellBias, cell));
    row[2] = __float_as_uint(occupancy_centre(d_key_z(k) - kCellBias, cell));
    row[3] = hits[j], row[4] = passes[j], row[5] = state[j];
}

__global__ void k_occupancy_extent_init(int32_t* extent) {
    if (blockIdx.x == 0 && threadIdx.x == 0) extent[OE_X_MIN] = INT_MAX, extent[OE_Y_MIN] = INT_MAX, extent[OE_X_MAX] = INT_MIN, extent[OE_Y_MAX] = INT_MIN;
}

__global__ __launch_bounds__(kBlock) void k_occupancy_extent(const unsigned long long* __restrict__ key, const int64_t m, const int32_t cz_lo, const int32_t cz_hi,
                                                             int32_t* extent) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int x_lo = INT_MAX, y_lo = INT_MAX, x_hi = INT_MIN, y_hi = INT_MIN;
    bool in = false;
    if (j < m) {
        const unsigned long long k = key[j];
        const int z = d_key_z(k);
        if (z >= cz_lo && z <= cz_hi) in = true, x_lo = x_hi = d_key_x(k), y_lo = y_hi = d_key_y(k);
    }
    if (__ballot(in) == 0ull) return;
    x_lo = wave_allmin(x_lo), y_lo = wave_allmin(y_lo), x_hi = wave_allmax(x_hi), y_hi = wave_allmax(y_hi);
    if ((threadIdx.x & 63) == 0) {
        // an extent only ever widens: a wave whose box lies inside what it reads has nothing to add (tens of thousands of waves, four words)
        const auto seen = [&](const int word) { return __hip_atomic_load(extent + word, kAgentRelaxed, __HIP_MEMORY_SCOPE_AGENT); };
        if (x_lo < seen(OE_X_MIN)) atomicMin(extent + OE_X_MIN, x_lo);
        if (y_lo < seen(OE_Y_MIN)) atomicMin(extent + OE_Y_MIN, y_lo);
        if (x_hi > seen(OE_X_MAX)) atomicMax(extent + OE_X_MAX, x_hi);
        if (y_hi > seen(OE_Y_MAX)) atomicMax(extent + OE_Y_MAX, y_hi);
    }
}

__global__ __launch_bounds__(kBlock) void k_occupancy_columns(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ state, const int64_t m,
                                                              const int32_t cz_lo, const int32_t cz_hi, const int32_t x_min, const int32_t y_max, const int32_t width,
                                                              const int32_t height, uint32_t* image) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const unsigned long long k = key[j];
    const int z = d_key_z(k);
    if (z < cz_lo || z > cz_hi) return;
    const int col = d_key_x(k) - x_min, row = y_max - d_key_y(k);
    if (col < 0 || col >= width || row < 0 || row >= height) return;  // (never: the extents are of these cells)
    atomicOr(image + (int64_t)row * width + col, 1u << (state[j] & 3u));
}

__global__ __launch_bounds__(kBlock) void k_occupancy_pixels(const uint32_t* __restrict__ image, const int64_t n, uint8_t* __restrict__ pixels,
                                                             unsigned long long* __restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t s = 0xFFFFFFFFu;
    if (i < n) {
        const uint32_t bits = image[i];
        s = (bits & (1u << kOccupancyOccupied)) ? kOccupancyOccupied : (bits & (1u << kOccupancyFree)) ? kOccupancyFree : kOccupancyUnknown;
        pixels[i] = s == kOccupancyOccupied ? (uint8_t)0 : s == kOccupancyFree ? (uint8_t)254 : (uint8_t)205;
    }
    d_count_lanes(s == kOccupancyUnknown, sums + OS_UNKNOWN);
    d_count_lanes(s == kOccupancyFree, sums + OS_FREE);
    d_count_lanes(s == kOccupancyOccupied, sums + OS_OCCUPIED);
}

}  // namespace

void launch_occupancy_clear(OccupancySlot* table, uint64_t slots, hipStream_t s) {
    if (slots > 0) hipLaunchKernelGGL(k_occupancy_clear, dim3(blocks_for(slots)), dim3(kBlock), 0, s, table, (unsigned long long)slots);
}
void launch_occupancy_walk(const GridView& grid, const float4* origin, OccupancyParams p, OccupancySlot* table, uint32_t mask, uint64_t limit, unsigned long long* rec,
                           hipStream_t s) {
    if (grid.n > 0)
        hipLaunchKernelGGL(k_occupancy_walk, dim3(blocks_for(grid.n)), dim3(kBlock), 0, s, grid.pts_sorted, grid.idx_sorted, origin, grid.n, p, table, mask,
                           (unsigned long long)limit, rec);
}
void launch_occupancy_flags(const OccupancySlot* table, uint64_t slots, int32_t* flag, hipStream_t s) {
    hipLaunchKernelGGL(k_occupancy_flags, dim3(blocks_for(slots + 1)), dim3(kBlock), 0, s, table, (unsigned long long)slots, flag);
}
void launch_occupancy_compact(const OccupancySlot* table, uint64_t slots, const int32_t* flag, const int32_t* scan, int64_t m, unsigned long long* key, uint32_t* slot_of,
                              hipStream_t s) {
    if (slots > 0) hipLaunchKernelGGL(k_occupancy_compact, dim3(blocks_for(slots)), dim3(kBlock), 0, s, table, (unsigned long long)slots, flag, scan, m, key, slot_of);
}
void launch_occupancy_states(const OccupancySlot* table, const uint32_t* slot_sorted, int64_t m, OccupancyParams p, uint32_t* hits, uint32_t* passes, uint32_t* state,
                             unsigned long long* sums, hipStream_t s) {
    if (m > 0) hipLaunchKernelGGL(k_occupancy_states, dim3(blocks_for(m)), dim3(kBlock), 0, s, table, slot_sorted, m, p, hits, passes, state, sums);
}
void launch_occupancy_select_flags(const uint32_t* state, int64_t m, uint32_t min_state, int32_t* keep, hipStream_t s) {
    hipLaunchKernelGGL(k_occupancy_select_flags, dim3(blocks_for((unsigned long long)m + 1)), dim3(kBlock), 0, s, state, m, min_state, keep);
}
void launch_occupancy_select(const int32_t* keep, const int32_t* scan, int64_t m, uint32_t* sel, hipStream_t s) {
    if (m > 0) hipLaunchKernelGGL(k_occupancy_select, dim3(blocks_for(m)), dim3(kBlock), 0, s, keep, scan, m, sel);
}
void launch_occupancy_rows(const unsigned long long* key, const uint32_t* hits, const uint32_t* passes, const uint32_t* state, const uint32_t* sel, int64_t first,
                           int64_t count, double cell, uint32_t* out, hipStream_t s) {
    if (count > 0) hipLaunchKernelGGL(k_occupancy_rows, dim3(blocks_for(count)), dim3(kBlock), 0, s, key, hits, passes, state, sel, first, count, cell, out);
}
void launch_occupancy_extent_init(int32_t* extent, hipStream_t s) { hipLaunchKernelGGL(k_occupancy_extent_init, dim3(1), dim3(64), 0, s, extent); }
void launch_occupancy_extent(const unsigned long long* key, int64_t m, int32_t cz_lo, int32_t cz_hi, int32_t* extent, hipStream_t s) {
    if (m > 0) hipLaunchKernelGGL(k_occupancy_extent, dim3(blocks_for(m)), dim3(kBlock), 0, s, key, m, cz_lo, cz_hi, extent);
}
void launch_occupancy_columns(const unsigned long long* key, const uint32_t* state, int64_t m, int32_t cz_lo, int32_t cz_hi, int32_t x_min, int32_t y_max, int32_t width,
                              int32_t height, uint32_t* image, hipStream_t s) {
    if (m > 0) hipLaunchKernelGGL(k_occupancy_columns, dim3(blocks_for(m)), dim3(kBlock), 0, s, key, state, m, cz_lo, cz_hi, x_min, y_max, width, height, image);
}
void launch_occupancy_pixels(const uint32_t* image, int64_t n, uint8_t* pixels, unsigned long long* sums, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_occupancy_pixels, dim3(blocks_for(n)), dim3(kBlock), 0, s, image, n, pixels, sums);
}

}  // namespace dmsa
