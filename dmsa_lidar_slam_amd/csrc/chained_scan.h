// chained_scan.h — the single-pass chained prefix scan ("decoupled look-back"), stated once for k_scan_i32 (radix_sort.hip),
// k_leaf_segments and k_leaf_finalize (dmsa_kernels.hip).  Device-only, everything __forceinline__, like wave_prims.h.
// A workgroup takes a tile by an atomic ticket, scans its rows, and chains to the tiles in front of it through one entry per tile in
// global memory: the tile publishes its K totals as PARTIAL, wave 0 walks the earlier entries until it has met a PREFIX, then the tile
// publishes its own inclusive prefix.  What a kernel keeps is how an element is loaded, what is written, and the FORMAT of an entry:
//     TileEntry<K> read(int64_t tile) const;                        // one entry, as it is now (absent / partial / prefix and K values)
//     void publish(uint32_t tile, int state, int q, int v) const;   // value q of this tile's entry, in state kTilePartial or kTilePrefix
// Both use __ATOMIC_RELAXED at __HIP_MEMORY_SCOPE_AGENT: an entry carries its values in the words that say it is there, so nothing else
// has to be ordered with it.  A format whose entry spans several words reports a state only when all words of that state are there.
#pragma once
#include <hip/hip_runtime.h>

#include "wave_prims.h"

namespace dmsa {

enum : int { kTileAbsent = 0, kTilePartial = 1, kTilePrefix = 2 };
template <int K>
struct TileEntry {
    int state;
    int v[K];
};
// what a workgroup of kWaves waves shares while it scans a tile of K values side by side
template <int K, int kWaves>
struct ChainedScanLds {
    int wave_total[kWaves][K];  // (first: every thread reads all of it, four words per instruction)
    int excl[K];
    uint32_t tile;
};

// Tiles in ticket order, not in blockIdx order: state[0] counts the tickets of all calls on this state, ticket_base is what it held when
// this call started (ChainedScanState in dmsa_ctx.h; 0 for a state that is cleared per call).
template <int K, int kWaves>
__device__ __forceinline__ uint32_t chained_scan_take_tile(ChainedScanLds<K, kWaves>& lds, unsigned long long* state, uint32_t ticket_base) {
    if (threadIdx.x == 0) lds.tile = atomicAdd(reinterpret_cast<unsigned int*>(state), 1u) - ticket_base;
    __syncthreads();
    return lds.tile;
}

// One row of 64 of a wave's rows: the inclusive prefix of x over this row and the wave's earlier rows; `run` carries the rows' sum.
__device__ __forceinline__ int chained_scan_row(int x, int& run) {
    const int sc = wave_incl_scan_dpp(x);
    const int incl = run + sc;
    run += __builtin_amdgcn_readlane(sc, 63);
    return incl;
}

// The look-back, by one wave: lane u inspects predecessor t - u, 64 tiles per round trip (a round trip to the device-coherent level of
// the cache hierarchy costs about a microsecond on this multi-die GPU, so the chain is walked as wide as possible).  A negative index
// reads as a prefix of zeros.  Adds to excl the sum of everything in front of `tile`.
// Forward progress: a ticket is only taken by a workgroup that is running, and a running workgroup publishes its partial totals without
// waiting for anyone.  So every predecessor of a tile is running or done, its entry appears whatever the others do, and tile 0 waits
// for nothing: the walk ends without any assumption about the order in which workgroups are started.
template <int K, class Format>
__device__ __forceinline__ void chained_look_back(const Format& fmt, uint32_t tile, int (&excl)[K]) {
    const int lane = threadIdx.x & 63;
    int64_t t = (int64_t)tile - 1;
    while (true) {
        const int64_t mine = t - lane;
        TileEntry<K> e = {kTilePrefix, {}};
        if (mine >= 0) e = fmt.read(mine);
        const unsigned long long ready = __ballot(e.state != kTileAbsent), prefix = __ballot(e.state == kTilePrefix);
        // lanes 0 .. stop-1 are consumed: up to and including the first prefix, or up to the first entry that is not there yet
        const int first_missing = ready == ~0ull ? 64 : __builtin_ctzll(~ready);
        const int first_prefix = prefix == 0ull ? 64 : __builtin_ctzll(prefix);
        const bool done = first_prefix < first_missing;
        const int stop = done ? first_prefix + 1 : first_missing;
#pragma unroll
        for (int q = 0; q < K; ++q) excl[q] += __builtin_amdgcn_readlane(wave_incl_scan_dpp(lane < stop ? e.v[q] : 0), 63);
        if (done) break;
        t -= stop;
    }
}

// The block step and the chain.  In: run[q], the sum of the calling wave's rows (chained_scan_row).  Out: off[q], everything in front of
// the wave's first row (earlier tiles + earlier waves of this tile), and upto[q], the inclusive prefix of the whole tile.
// Publishing is two stores by lanes 0 .. K-1 of wave 0, lane q with value q: partial before the walk, prefix after it (tile 0 is its
// own prefix at once).
template <int K, int kWaves, class Format>
__device__ __forceinline__ void chained_scan_tile(ChainedScanLds<K, kWaves>& lds, const Format& fmt, uint32_t tile, const int (&run)[K], int (&off)[K],
                                                  int (&upto)[K]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;  // (loops over q: K <= 2, unrolled without being told)
    for (int q = 0; q < K; ++q)
        if (lane == 0) lds.wave_total[wave][q] = run[q];
    __syncthreads();
    int before[K] = {}, total[K] = {};
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
#pragma unroll
        for (int q = 0; q < K; ++q) {
            const int t = lds.wave_total[w][q];
            if (w < wave) before[q] += t;
            total[q] += t;
        }
    if (wave == 0) {
        int excl[K] = {}, mine = 0;  // lane q publishes value q
        for (int q = 0; q < K; ++q) mine = lane == q ? total[q] : mine;
        if (tile != 0) {
            if (lane < K) fmt.publish(tile, kTilePartial, lane, mine);
            chained_look_back<K>(fmt, tile, excl);
        }
        for (int q = 0; q < K; ++q) mine += lane == q ? excl[q] : 0;
        if (lane < K) fmt.publish(tile, kTilePrefix, lane, mine);
        for (int q = 0; q < K; ++q)
            if (lane == 0) lds.excl[q] = excl[q];
    }
    __syncthreads();
    for (int q = 0; q < K; ++q) off[q] = lds.excl[q] + before[q], upto[q] = lds.excl[q] + total[q];
}

}  // namespace dmsa
