// dense_carve.hip — the kernels of include/dmsa_dense_carve.h: moving objects removed from the dense cloud by ray carving.
//
//   k_carve_passes      T2-T6, the hot kernel: one ray per lane, walked from cell to cell with csrc/dense_carve_walk.h
//   k_carve_walk_rows   the stage call: the same walk, one thread per row, its length and hash
//   k_carve_flags       passes against min_passes, once all rays are counted
//
// k_carve_passes takes its rays in the grid's SORTED row order: the 64 rays of a wave end in the same few cells and start from nearly the same
// origin, so their walks run through neighbouring cells.  A lane keeps the walk of T4 in registers (CarveWalk: six int64, nine int32, no
// array), makes one d_cell_slot probe per traversed cell and streams the cell's run of sorted rows through T5.  A ray that sees through a row
// adds 1 to that row's count with a plain vector atomicAdd; the four statistics are summed in the wave and added with one 64-bit vector
// atomicAdd per sum and wave.  Integer sums: the result does not depend on the order.  No LDS.  Built with -ffp-contract=off.
#include "dense_carve.h"

#include "dense_carve_walk.h"
#include "dense_grid_walk.h"

namespace dmsa {
namespace {

__global__ __launch_bounds__(kBlock) void k_carve_passes(const float4* __restrict__ pts, const uint32_t* __restrict__ idx, const float4* __restrict__ origin,
                                                         const int64_t n, const DenseCellEntry* __restrict__ table, const uint32_t mask, const CarveParams p,
                                                         uint32_t* __restrict__ passes, unsigned long long* __restrict__ sums) {
    const int64_t self = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // this lane's sorted row: its ray
    unsigned long long skipped = 0ull, cells = 0ull, pairs = 0ull, seen = 0ull;
    if (self < n) {
        const float4 g = pts[self], o = origin[idx[self]];
        const CarveRay ray = carve_ray(o.x, o.y, o.z, g.x, g.y, g.z);
        const CarvePair pair = carve_pair(p.rho, p.tan_half_angle, p.end_margin, p.start_margin);
        CarveWalk w;
        if (carve_ray_skipped(ray, p.max_length) || !carve_walk_begin(p.cell, o.x, o.y, o.z, g.x, g.y, g.z, &w)) {
            skipped = 1ull;
        } else {
            const uint32_t me = (uint32_t)self, rows = (uint32_t)n;  // (n <= 2^26)
#pragma unroll 1
            for (int32_t step = 0; step <= kCarveMaxSteps; ++step) {  // (T4: the walk ends before the bound does)
                ++cells;
                if (carve_cell_holds_rows(w)) {
                    bool found;
                    const uint32_t slot = d_cell_slot(table, mask, d_cell_key(w.cx + kCellBias, w.cy + kCellBias, w.cz + kCellBias), &found);
                    if (found) {
                        uint32_t cs = table[slot].start, ce = table[slot].end;
                        if (ce > rows) ce = rows;  // (never: every cell's end was entered)
#pragma unroll 1
                        for (uint32_t j = cs; j < ce; ++j) {
                            if (j == me) continue;  // T5: j != r
                            ++pairs;
                            const float4 c = pts[j];
                            if (carve_sees_through(ray, pair, g.x, g.y, g.z, c.x, c.y, c.z)) {
                                ++seen;
                                atomicAdd(passes + idx[j], 1u);
                            }
                        }
                    }
                }
                if (!carve_walk_step(&w)) break;
            }
        }
    }
    skipped = wave_sum(skipped), cells = wave_sum(cells), pairs = wave_sum(pairs), seen = wave_sum(seen);
    if ((threadIdx.x & 63) == 0) {
        if (skipped != 0ull) atomicAdd(sums + CS_SKIPPED, skipped);
        if (cells != 0ull) atomicAdd(sums + CS_CELLS, cells);
        if (pairs != 0ull) atomicAdd(sums + CS_PAIRS, pairs);
        if (seen != 0ull) atomicAdd(sums + CS_SEEN, seen);
    }
}

__global__ __launch_bounds__(kBlock) void k_carve_walk_rows(const float4* __restrict__ g, const float4* __restrict__ origin, const int64_t first, const int64_t count,
                                                            const CarveParams p, int32_t* __restrict__ n_cells, unsigned long long* __restrict__ hash) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const float4 e = g[first + i], o = origin[first + i];
    const CarveRay ray = carve_ray(o.x, o.y, o.z, e.x, e.y, e.z);
    CarveWalk w;
    int32_t cells = -1;
    unsigned long long h = 0ull;
    if (!carve_ray_skipped(ray, p.max_length) && carve_walk_begin(p.cell, o.x, o.y, o.z, e.x, e.y, e.z, &w)) {
        cells = 0, h = kCarveHashSeed;
#pragma unroll 1
        for (int32_t step = 0; step <= kCarveMaxSteps; ++step) {
            ++cells;
            h = carve_hash_cell(h, w);
            if (!carve_walk_step(&w)) break;
        }
    }
    n_cells[i] = cells;
    hash[i] = h;
}

__global__ __launch_bounds__(kBlock) void k_carve_flags(const uint32_t* __restrict__ passes, const int64_t n, const uint32_t min_passes, int32_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    keep[i] = i < n && passes[i] < min_passes ? 1 : 0;
}

}  // namespace

void launch_carve_walk_rows(const float4* g, const float4* origin, int64_t first, int64_t count, CarveParams p, int32_t* n_cells, unsigned long long* hash, hipStream_t s) {
    if (count > 0) hipLaunchKernelGGL(k_carve_walk_rows, dim3(blocks_for(count)), dim3(kBlock), 0, s, g, origin, first, count, p, n_cells, hash);
}
void launch_carve_passes(const GridView& grid, const float4* origin, CarveParams p, uint32_t* passes, unsigned long long* sums, hipStream_t s) {
    if (grid.n > 0)
        hipLaunchKernelGGL(k_carve_passes, dim3(blocks_for(grid.n)), dim3(kBlock), 0, s, grid.pts_sorted, grid.idx_sorted, origin, grid.n, grid.table, grid.mask, p, passes,
                           sums);
}
void launch_carve_flags(const uint32_t* passes, int64_t n, uint32_t min_passes, int32_t* keep, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_carve_flags, dim3(blocks_for((unsigned long long)n + 1)), dim3(kBlock), 0, s, passes, n, min_passes, keep);
}

}  // namespace dmsa
