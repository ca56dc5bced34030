// dense_clusters.h — launchers of the kernels behind include/dmsa_dense_clusters.h (csrc/dense_clusters.hip): a lock-free union-find over the
// sorted rows of the search grid of csrc/dense_grid.h, the smallest store row and the size of every cluster, and the flags and sums of a
// classification.  The compaction and the rows of the file are the kernels of csrc/dense_cloud.h.
#pragma once
#include "dense_grid.h"

namespace dmsa {

// the words of the sums block in HBM, zeroed before the first launch of a call
enum ClusterSum { CL_CLUSTERS = 0, CL_LARGEST, CL_KEPT_ROWS, CL_KEPT_CLUSTERS, CL_SMALL, CL_LARGE, CL_GAVE_UP, CL_COUNT };
// CL_GAVE_UP: a loop of the union-find ran into its bound (never on a correct build: dense_clusters.hip)
constexpr unsigned long long kClusterGaveUpFind = 1ull, kClusterGaveUpHook = 2ull;

// parent[s] = s, min_row[s] = INT32_MAX, count[s] = 0 for the n sorted rows
void launch_cluster_init(int64_t n, uint32_t* parent, int32_t* min_row, int32_t* count, hipStream_t s);
// C2: every pair of adjacent rows united in `parent` (sorted-row space; the larger root hooks under the smaller)
void launch_cluster_link(const GridView& grid, float r2, uint32_t* parent, unsigned long long* sums, hipStream_t s);
// root[s] = the root of s in `parent` (whose paths the walks shorten); min_row[root] = the smallest store row under that root
void launch_cluster_flatten(const GridView& grid, uint32_t* parent, uint32_t* root, int32_t* min_row, unsigned long long* sums, hipStream_t s);
// count[root] = the rows under that root
void launch_cluster_sizes(int64_t n, const uint32_t* root, int32_t* count, hipStream_t s);
// C3 in store-row terms: label[idx_sorted[s]] = min_row[root[s]], size[idx_sorted[s]] = count[root[s]]
void launch_cluster_rows(const GridView& grid, const uint32_t* root, const int32_t* min_row, const int32_t* count, int32_t* label, int32_t* size, hipStream_t s);
// C4-C5: keep[i] = flag8[i] = C4 of size[i]; keep[n] = 0 (the scan over n + 1 flags ends in the rows kept); sums[CL_CLUSTERS .. CL_LARGE] +=
// this launch's share (CL_LARGEST: a maximum)
void launch_cluster_flags(const int32_t* label, const int32_t* size, int64_t n, int32_t min_size, int32_t max_size, int32_t* keep, uint8_t* flag8,
                          unsigned long long* sums, hipStream_t s);

}  // namespace dmsa
