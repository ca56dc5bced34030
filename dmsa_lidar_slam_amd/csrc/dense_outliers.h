// dense_outliers.h — launchers of the kernels behind include/dmsa_dense_outliers.h (csrc/dense_outliers.hip): the mean distance of every
// retained row to its k nearest neighbours over the search grid of csrc/dense_grid.h, the exact cloud-wide sums, and the flags against the
// threshold.  The compaction and the 12-byte rows of the file are the kernels of csrc/dense_cloud.h.
#pragma once
#include "dense_grid.h"

namespace dmsa {

constexpr int kOutlierMaxK = 16;  // O1; the largest capacity k_knn_mean_distance is instantiated for
// the words of the sums block in HBM, zeroed before k_outlier_quantise_sum
enum OutlierSum { OS_N = 0, OS_S1, OS_S2, OS_ISOLATED, OS_COUNT };

// O2-O3 for the retained rows [first, first + count): mean[row - first] = m_i, a quiet NaN for an isolated row.  1 <= k <= kOutlierMaxK.
void launch_knn_mean_distance(const GridView& grid, float r2, int32_t k, int64_t first, int64_t count, float* mean, hipStream_t s);
// O4: q[i] = (int32)rintf(mean[i] * scale), -1 for an isolated row; sums[OS_N .. OS_ISOLATED] += this launch's share
void launch_outlier_quantise_sum(const float* mean, int64_t n, float scale, int32_t* q, unsigned long long* sums, hipStream_t s);
// O5: keep[i] = flag8[i] = (q[i] >= 0 && (double)q[i] <= threshold); keep[n] = 0 (the scan over n + 1 flags ends in the number of inliers)
void launch_outlier_flags(const int32_t* q, int64_t n, double threshold, int32_t* keep, uint8_t* flag8, hipStream_t s);

}  // namespace dmsa
