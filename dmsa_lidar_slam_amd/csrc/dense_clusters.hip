// dense_clusters.hip — the kernels of include/dmsa_dense_clusters.h: Euclidean clusters of the dense cloud as connected components.
//
//   k_cluster_init      every sorted row its own root
//   k_cluster_link      C2, the hot kernel: the traversal of csrc/dense_grid_walk.h; every adjacent pair is united once
//   k_cluster_flatten   root[s] = the root of s, and the smallest store row under every root (an integer atomicMin)
//   k_cluster_sizes     the rows under every root (an integer atomicAdd)
//   k_cluster_rows      C3 in store-row terms: label and size of every row
//   k_cluster_flags     C4's flags and C5's sums (a wave reduction, then plain 64-bit vector atomics)
//
// The union-find lives in SORTED-row space: a row's neighbours are near it in the sorted order, so the words of `parent` a wave touches lie
// close together.  It is lock-free and order-free:
//   * a hook is one atomicCAS on a ROOT's own slot, parent[hi]: hi -> lo with lo < hi.  So parent[x] <= x always, parent[x] < x for every
//     row that is no root, a row that stopped being a root never becomes one again, and the forest has no cycle whatever order the hooks
//     land in.  When every pair has been united the root of a component is its smallest sorted row: a fact about the graph, not the schedule.
//   * d_find halves paths with plain relaxed stores of a grandparent.  They touch only rows that are no roots, and whatever value wins a
//     race is an ancestor of the row and smaller than it.
//   * parent is read and written with relaxed agent-scope atomics only (loads and stores that bypass the CU's L1, which another CU's stores
//     never refresh).  A stale value is an older ancestor: the walk is longer, never wrong.  The CAS decides.
//   * no lane ever waits for another lane's progress.  EVERY LOOP HAS A BOUND: a walk's row index falls strictly with every hop and the
//     larger of a hook's two roots falls strictly with every failed CAS, so n is a bound for both; a lane that exhausts one sets a bit of
//     sums[CL_GAVE_UP] and leaves, and the host turns the bit into an error.  That cannot happen on a correct build.
//   * the flattening writes the roots into an array of their own: a walk that halves paths may store an older ancestor into ANY row on
//     its way, so `parent` itself is flat only where no other lane's walk passed last.
// The phases are separated by kernel boundaries.  Labels in store-row terms come from an atomicMin over the store rows of every root:
// integer and order-free like the sizes.  Built with -ffp-contract=off (C2 is N2's expression, operation for operation).
#include "dense_clusters.h"

#include "dense_grid_walk.h"

#include <climits>

namespace dmsa {
namespace {

constexpr uint32_t kNoRoot = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t d_parent(const uint32_t* parent, const uint32_t x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void d_set_parent(uint32_t* parent, const uint32_t x, const uint32_t v) {
    __hip_atomic_store(parent + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void d_give_up(unsigned long long* sums, const unsigned long long which) { atomicOr(sums + CL_GAVE_UP, which); }

// the root of x, halving the path on the way (x skips to its grandparent); kNoRoot after n hops
__device__ __forceinline__ uint32_t d_find(uint32_t* parent, uint32_t x, const uint32_t n, unsigned long long* sums) {
#pragma unroll 1
    for (uint32_t hop = 0; hop < n; ++hop) {
        const uint32_t p = d_parent(parent, x);
        if (p == x) return x;
        const uint32_t gp = d_parent(parent, p);
        if (gp == p) return p;
        d_set_parent(parent, x, gp);  // (x is no root: p != x)
        x = gp;                       // gp < p < x
    }
    d_give_up(sums, kClusterGaveUpFind);
    return kNoRoot;
}

// the trees of a and b made one; returns their common root as it was at that moment (a itself once a loop has given up)
__device__ __forceinline__ uint32_t d_unite(uint32_t* parent, const uint32_t a, const uint32_t b, const uint32_t n, unsigned long long* sums) {
    uint32_t ra = d_find(parent, a, n, sums), rb = d_find(parent, b, n, sums);
#pragma unroll 1
    for (uint32_t round = 0; round < n; ++round) {
        if (ra == kNoRoot || rb == kNoRoot) return a;
        if (ra == rb) return ra;
        const uint32_t hi = max(ra, rb), lo = min(ra, rb);
        uint32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return lo;
        ra = d_find(parent, seen, n, sums);  // hi is no root any more: on from the parent the CAS saw, which is below hi
        rb = d_find(parent, lo, n, sums);
    }
    d_give_up(sums, kClusterGaveUpHook);
    return a;
}

__global__ __launch_bounds__(kBlock) void k_cluster_init(const int64_t n, uint32_t* __restrict__ parent, int32_t* __restrict__ min_row, int32_t* __restrict__ count) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    parent[s] = (uint32_t)s, min_row[s] = INT_MAX, count[s] = 0;
}

__global__ __launch_bounds__(kBlock) void k_cluster_link(const float4* __restrict__ pts, const unsigned long long* __restrict__ key, const int64_t n,
                                                         const DenseCellEntry* __restrict__ table, const uint32_t mask, const float r2, uint32_t* parent,
                                                         unsigned long long* sums) {
    const int lane = threadIdx.x & 63;
    const int64_t self = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 64 + lane;  // this lane's sorted row
    const bool live = self < n;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    unsigned long long my_key = kCellEmptyKey;
    if (live) {
        const float4 p = pts[self];
        qx = p.x, qy = p.y, qz = p.z;
        my_key = key[self];
    }
    if (__ballot(live) == 0ull) return;  // (the whole wave)
    const uint32_t me = (uint32_t)self, rows = (uint32_t)n;  // (n <= 2^26)
    uint32_t known = me;  // an ancestor of `me` (or the row itself): where the next walk starts
    d_walk_candidates(pts, n, table, mask, lane, live, my_key, [&](const bool mine, const float x, const float y, const float z, const uint32_t j) {
        const float dx = x - qx, dy = y - qy, dz = z - qz;
        float d2 = dx * dx;
        d2 += dy * dy;
        d2 += dz * dz;
        // the pair (me, j) belongs to the lane with the higher sorted row: every edge is united once
        if (mine && d2 <= r2 && j < me && d_parent(parent, j) != known) known = d_unite(parent, known, j, rows, sums);
    });
}

__global__ __launch_bounds__(kBlock) void k_cluster_flatten(const uint32_t* __restrict__ idx, const int64_t n, uint32_t* parent, uint32_t* __restrict__ root_of,
                                                            int32_t* min_row, unsigned long long* sums) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = s < n;
    uint32_t root = kNoRoot;
    int32_t row = INT_MAX;
    if (live) {
        root = d_find(parent, (uint32_t)s, (uint32_t)n, sums);
        row = (int32_t)idx[s];
        root_of[s] = root != kNoRoot ? root : (uint32_t)s;  // (a row of the store whatever happened: the host reads the give-up word)
    }
    const bool found = live && root != kNoRoot;
    // consecutive sorted rows mostly share their root: then one atomic serves the wave
    const unsigned long long act = __ballot(found);
    if (act == 0ull) return;
    const int first = __ffsll((long long)act) - 1;
    const uint32_t root0 = (uint32_t)__builtin_amdgcn_readlane((int)root, first);
    if (__ballot(found && root == root0) == act) {
        const int32_t lowest = wave_allmin(found ? row : INT_MAX);
        if ((threadIdx.x & 63) == first) atomicMin(min_row + root0, lowest);
    } else if (found) {
        atomicMin(min_row + root, row);
    }
}

__global__ __launch_bounds__(kBlock) void k_cluster_sizes(const int64_t n, const uint32_t* __restrict__ root_of, int32_t* count) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = s < n;
    const uint32_t root = live ? root_of[s] : kNoRoot;
    const unsigned long long act = __ballot(live);
    if (act == 0ull) return;
    const int first = __ffsll((long long)act) - 1;
    const uint32_t root0 = (uint32_t)__builtin_amdgcn_readlane((int)root, first);
    if (__ballot(live && root == root0) == act) {
        if ((threadIdx.x & 63) == first) atomicAdd(count + root0, (int32_t)__popcll(act));
    } else if (live) {
        atomicAdd(count + root, 1);
    }
}

__global__ __launch_bounds__(kBlock) void k_cluster_rows(const uint32_t* __restrict__ idx, const int64_t n, const uint32_t* __restrict__ root_of,
                                                         const int32_t* __restrict__ min_row, const int32_t* __restrict__ count, int32_t* __restrict__ label,
                                                         int32_t* __restrict__ size) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const uint32_t root = root_of[s], row = idx[s];
    label[row] = min_row[root], size[row] = count[root];
}

__global__ __launch_bounds__(kBlock) void k_cluster_flags(const int32_t* __restrict__ label, const int32_t* __restrict__ size, const int64_t n, const int32_t min_size,
                                                          const int32_t max_size, int32_t* __restrict__ keep, uint8_t* __restrict__ flag8,
                                                          unsigned long long* __restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long heads = 0ull, largest = 0ull, kept = 0ull, kept_heads = 0ull, small = 0ull, large = 0ull;
    if (i < n) {
        const int32_t sz = size[i];
        const bool head = label[i] == (int32_t)i, is_small = sz < min_size, is_large = max_size != 0 && sz > max_size;  // (never both: min_size <= max_size)
        const bool in = !is_small && !is_large;
        keep[i] = in ? 1 : 0;
        flag8[i] = in ? 1 : 0;
        heads = head ? 1ull : 0ull, largest = (unsigned long long)sz, kept = in ? 1ull : 0ull, kept_heads = head && in ? 1ull : 0ull;
        small = is_small ? 1ull : 0ull, large = is_large ? 1ull : 0ull;
    } else if (i == n) {
        keep[n] = 0;
    }
    heads = wave_sum(heads), kept = wave_sum(kept), kept_heads = wave_sum(kept_heads), small = wave_sum(small), large = wave_sum(large);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) largest = max(largest, __shfl_xor(largest, o));
    if ((threadIdx.x & 63) == 0) {
        if (heads != 0ull) atomicAdd(sums + CL_CLUSTERS, heads);
        if (largest != 0ull) atomicMax(sums + CL_LARGEST, largest);
        if (kept != 0ull) atomicAdd(sums + CL_KEPT_ROWS, kept);
        if (kept_heads != 0ull) atomicAdd(sums + CL_KEPT_CLUSTERS, kept_heads);
        if (small != 0ull) atomicAdd(sums + CL_SMALL, small);
        if (large != 0ull) atomicAdd(sums + CL_LARGE, large);
    }
}

}  // namespace

void launch_cluster_init(int64_t n, uint32_t* parent, int32_t* min_row, int32_t* count, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_cluster_init, dim3(blocks_for(n)), dim3(kBlock), 0, s, n, parent, min_row, count);
}
void launch_cluster_link(const GridView& g, float r2, uint32_t* parent, unsigned long long* sums, hipStream_t s) {
    if (g.n > 0) hipLaunchKernelGGL(k_cluster_link, dim3(blocks_for(g.n)), dim3(kBlock), 0, s, g.pts_sorted, g.key_sorted, g.n, g.table, g.mask, r2, parent, sums);
}
void launch_cluster_flatten(const GridView& g, uint32_t* parent, uint32_t* root, int32_t* min_row, unsigned long long* sums, hipStream_t s) {
    if (g.n > 0) hipLaunchKernelGGL(k_cluster_flatten, dim3(blocks_for(g.n)), dim3(kBlock), 0, s, g.idx_sorted, g.n, parent, root, min_row, sums);
}
void launch_cluster_sizes(int64_t n, const uint32_t* root, int32_t* count, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_cluster_sizes, dim3(blocks_for(n)), dim3(kBlock), 0, s, n, root, count);
}
void launch_cluster_rows(const GridView& g, const uint32_t* root, const int32_t* min_row, const int32_t* count, int32_t* label, int32_t* size, hipStream_t s) {
    if (g.n > 0) hipLaunchKernelGGL(k_cluster_rows, dim3(blocks_for(g.n)), dim3(kBlock), 0, s, g.idx_sorted, g.n, root, min_row, count, label, size);
}
void launch_cluster_flags(const int32_t* label, const int32_t* size, int64_t n, int32_t min_size, int32_t max_size, int32_t* keep, uint8_t* flag8,
                          unsigned long long* sums, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_cluster_flags, dim3(blocks_for((unsigned long long)n + 1)), dim3(kBlock), 0, s, label, size, n, min_size, max_size, keep, flag8, sums);
}

}  // namespace dmsa
