// dense_grid_walk.h — the device side of the search grid over the retained rows (csrc/dense_grid.h), stated once for the kernels that build it
// (csrc/dense_grid.hip) and those that walk it: k_neighbour_moments (csrc/dense_normals.hip), k_knn_mean_distance (csrc/dense_outliers.hip)
// and, cell by cell, k_carve_passes (csrc/dense_carve.hip).  Wave helpers: wave_prims.h.  Device code only.
//
// d_walk_candidates: a WAVE owns 64 consecutive sorted rows, one query per lane.  It takes the box of its queries' cells grown by one cell,
// looks the box's cells up 64 at a time (a lane per cell), merges cells whose runs of sorted rows touch (cells that are neighbours along z do)
// and streams the runs in tiles of kGridTile rows: every lane loads one candidate, and the wave walks the tile with v_readlane, so a
// candidate costs the wave three scalar reads and no LDS.  Every lane is offered every candidate of the box -- the caller's distance test is
// the definition, and a candidate two cells away fails it -- so each candidate is offered exactly once.  Where 64 consecutive rows span a
// box of more than kGridBoxCells cells (the sorted order jumps between surfaces) the wave goes through its distinct cells one by one with
// the 27 cells around each, the other lanes masked.
#pragma once
#include "dense_dev.h"
#include "dense_grid.h"
#include "wave_prims.h"

#include <climits>
#include <cmath>

namespace dmsa {

constexpr unsigned long long kCellEmptyKey = ~0ull;
constexpr int kCellBias = 1 << 20, kCellMax = (1 << 21) - 1;

__device__ __forceinline__ unsigned long long d_cell_key(const int x, const int y, const int z) {
    return ((unsigned long long)x << 42) | ((unsigned long long)y << 21) | (unsigned long long)z;
}
// the slot of `key` in the table, or of the empty slot that ends its probe sequence (the table is at most half full)
__device__ __forceinline__ uint32_t d_cell_slot(const DenseCellEntry* table, const uint32_t mask, const unsigned long long key, bool* found) {
    uint32_t slot = (uint32_t)mix64(key) & mask;
    *found = false;
#pragma unroll 1
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const unsigned long long kk = table[slot].key;
        if (kk == key) {
            *found = true;
            return slot;
        }
        if (kk == kCellEmptyKey) return slot;
        slot = (slot + 1) & mask;
    }
    return slot;
}

// Called by all 64 lanes of a wave of which at least one is `live` (my_key = the cell key of a live lane's query).  step(mine, x, y, z, j): the
// candidate is sorted row j at (x, y, z), the same in every lane; `mine` says whether this pass serves the lane's query.  Every loop bound is
// the same in all 64 lanes.
template <class Step>
__device__ __forceinline__ void d_walk_candidates(const float4* __restrict__ pts, const int64_t n, const DenseCellEntry* __restrict__ table, const uint32_t mask,
                                                  const int lane, const bool live, const unsigned long long my_key, Step step) {
    const unsigned long long act = __ballot(live);
    const int cx = (int)(my_key >> 42) & kCellMax, cy = (int)(my_key >> 21) & kCellMax, cz = (int)my_key & kCellMax;
    const auto lowest = [](const int v) { return __builtin_amdgcn_readfirstlane(wave_allmin(v)); };
    const auto highest = [](const int v) { return __builtin_amdgcn_readfirstlane(wave_allmax(v)); };
    const int lox = lowest(live ? cx : INT_MAX), loy = lowest(live ? cy : INT_MAX), loz = lowest(live ? cz : INT_MAX);
    const int hix = highest(live ? cx : INT_MIN), hiy = highest(live ? cy : INT_MIN), hiz = highest(live ? cz : INT_MIN);
    const bool whole = (unsigned long long)(hix - lox + 3) * (unsigned long long)(hiy - loy + 3) * (unsigned long long)(hiz - loz + 3) <=
                       (unsigned long long)kGridBoxCells;  // (each factor is at most 2^21 + 2: the product fits 64 bits)
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
                for (uint32_t t = rs; t < re; t += kGridTile) {
                    const uint32_t j = t + (uint32_t)lane;
                    float4 cand = make_float4(INFINITY, INFINITY, INFINITY, 0.0f);  // (d2 = inf: never a neighbour)
                    if (j < re) cand = pts[j];
                    const int held = (int)min((uint32_t)kGridTile, re - t);
                    for (int u = 0; u < held; ++u) step(mine, bcast_lane(cand.x, u), bcast_lane(cand.y, u), bcast_lane(cand.z, u), t + (uint32_t)u);
                }
                if (last) break;
                rs = ns, re = ne;
            }
        }
    }
}

}  // namespace dmsa
