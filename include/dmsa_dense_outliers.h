/*
 * dmsa_dense_outliers.h — C ABI of statistical outlier removal for the dense cloud (include/dmsa_dense_cloud.h): the mean distance of every
 * retained point to its k nearest neighbours, a cloud-wide threshold mean + stddev_mul * stddev over those means, and the retained store
 * (include/dmsa_dense_normals.h, N0) compacted to the points below it.  What PCL's StatisticalOutlierRemoval and CloudCompare's "SOR" do,
 * on the points where they already are.
 *
 * Like the rules 1-7 and N0-N5 the semantics are DECIDED HERE, stated below, and tested against an independent numpy model
 * (tests/dense_outliers_model.py).  They are chosen so that the result does not depend on how the work is split over lanes, waves or
 * atomics: the same input gives the same bytes on every run.  Same conventions as dmsa_hip.h (contexts, status codes, no CPU fallback).
 *
 * O1  PRECONDITIONS, else DMSA_ERR_INVALID with the reason in dmsa_last_error: everything N1 asks of `radius` (retention on, at least one
 *     retained row, voxel_size > 0, radius finite and in [voxel_size, 64 * voxel_size]); 1 <= k <= 16 (at the workload's ratio, radius = 3
 *     voxels, a surface holds about 28 rows in the ball: a larger k mostly declares isolation); stddev_mul finite and >= 0; retained rows
 *     <= 2^26 (this keeps the sums of O4 inside int64).
 * O2  CANDIDATES of row i: every retained row j != i (by row index, not by distance) with d2 <= radius * radius, d2 being N2's float
 *     expression, operation for operation.
 * O3  MEAN DISTANCE.  The k smallest d2 among the candidates, as a multiset: only the values are used, so ties need no rule.  Fewer than k
 *     candidates: the row is ISOLATED and m_i is a quiet NaN.  Otherwise, in float, each operation rounded on its own,
 *     m_i = (((sqrtf(d2_(1)) + sqrtf(d2_(2))) + ...) + sqrtf(d2_(k))) / (float)k, in ascending order of d2.
 * O4  EXACT STATISTICS.  frexpf(radius) = m * 2^e; scale = 2^(18 - e).  q_i = (int64)rintf(m_i * scale): the product is exact and
 *     q_i <= 2^18.  Over the non-isolated rows three int64 sums: n_s, S1 = sum q_i, S2 = sum q_i^2 (<= 2^62).  Integer addition is
 *     associative: any split gives the same three integers.
 * O5  THRESHOLD, on the host, in double, each operation rounded on its own, in PCL's form of the formula:
 *     mean = (double)S1 / (double)n_s; var = ((double)S2 - ((double)S1 * (double)S1) / (double)n_s) / (double)(n_s - 1); var = 0 if n_s < 2
 *     or var < 0; T = mean + (double)stddev_mul * sqrt(var).  Row i is an INLIER iff it is not isolated and (double)q_i <= T.  Isolated rows
 *     are always outliers.  n_s == 0: every row is isolated and T = 0.
 * O6  THE STORE.  A classification stays valid until a scan is added.  dmsa_dense_cloud_remove_outliers compacts the retained points AND
 *     their origins to the inliers, stably, in store order; the classification, the search grid and any normals are then invalid.  The voxel
 *     set is NOT touched: a voxel that held an outlier stays taken for later scans.  dmsa_dense_stats is not touched either: it counts what
 *     the scans kept.  dmsa_dense_cloud_compute_normals / save_pcd_normals afterwards work on the cleaned store, because it IS the store.
 */
#ifndef DMSA_DENSE_OUTLIERS_H
#define DMSA_DENSE_OUTLIERS_H

#include "dmsa_dense_normals.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmsa_dense_outlier_config {
    float   radius;      /* 0.3: metres; the reach of the neighbour search (O2)   */
    int32_t k;           /* 8:   neighbours per mean, 1 .. 16                     */
    float   stddev_mul;  /* 1.0: T = mean + stddev_mul * stddev; finite, >= 0     */
    int32_t pad;
} dmsa_dense_outlier_config;
void dmsa_default_dense_outlier_config(dmsa_dense_outlier_config* cfg);

typedef struct dmsa_dense_outlier_stats {
    int64_t rows, isolated, above_threshold, inliers; /* rows = isolated + above_threshold + inliers */
    int64_t n_s, s1, s2;                              /* O4                                          */
    double  mean_m, stddev_m, threshold_m;            /* O5's mean, sqrt(var) and T divided by scale: metres */
} dmsa_dense_outlier_stats;

/* The stage call of O2-O3: m_i of rows [first, first + count) into mean_out (count floats, NaN = isolated), as the kernel behind
 * dmsa_dense_cloud_classify_outliers computes them. */
int dmsa_dense_cloud_knn_mean_distance(dmsa_dense_cloud* dc, const dmsa_dense_outlier_config* cfg, int64_t first, int64_t count, float* mean_out);
/* O2-O5 for every retained row.  inlier_out (rows bytes, 1 = inlier, 0 = outlier) and stats may be NULL; the flags stay in HBM for
 * dmsa_dense_cloud_remove_outliers until the next scan is added. */
int dmsa_dense_cloud_classify_outliers(dmsa_dense_cloud* dc, const dmsa_dense_outlier_config* cfg, uint8_t* inlier_out, dmsa_dense_outlier_stats* stats);
/* Host only, no context: O5.  *threshold_q = T, *mean_q and *stddev_q = mean and sqrt(var), all in the units of q (any of the three may be
 * NULL).  n_s < 0, s1 < 0, s2 < 0, or a stddev_mul that is not finite or negative: DMSA_ERR_INVALID. */
int dmsa_dense_outlier_threshold(int64_t n_s, int64_t s1, int64_t s2, float stddev_mul, double* mean_q, double* stddev_q, double* threshold_q);
/* O6.  Needs a classification that is still valid (none yet, a scan added since, or the store already compacted by it: DMSA_ERR_INVALID).
 * *kept (optional) = rows left in the store. */
int dmsa_dense_cloud_remove_outliers(dmsa_dense_cloud* dc, int64_t* kept);
/* The retained store as it stands, as the x y z binary PCD of dmsa_pcd_header_xyz_binary: 12-byte rows in store order.  An empty store or a
 * path that cannot be written gives DMSA_ERR_INVALID and leaves no partial file.  *points_out / *bytes_out (optional) = rows in the file /
 * its size.  The streaming x y z file of dmsa_dense_cloud_open_pcd / close_pcd is independent of this. */
int dmsa_dense_cloud_save_pcd_retained(dmsa_dense_cloud* dc, const char* path, int64_t* points_out, int64_t* bytes_out);

#ifdef __cplusplus
}
#endif
#endif /* DMSA_DENSE_OUTLIERS_H */
