/*
 * dmsa_dense_clusters.h — C ABI of Euclidean clustering for the dense cloud (include/dmsa_dense_cloud.h): the connected components of the
 * retained store (include/dmsa_dense_normals.h, N0) under "two rows are at most `radius` apart", a label and a size per row, and the store
 * compacted to the rows of clusters inside a size range.  What PCL's EuclideanClusterExtraction and CloudCompare's "label connected
 * components" do, on the points where they already are.  It takes out what ray carving (include/dmsa_dense_carve.h) leaves of a moving
 * object and statistical outlier removal (include/dmsa_dense_outliers.h) cannot see: a small blob whose points are each other's neighbours.
 *
 * Like O1-O6 and T1-T7 the semantics are DECIDED HERE, stated below, and tested against an independent model
 * (tests/dense_clusters_model.py).  They are chosen so that the result does not depend on how lanes, waves or atomics interleave: the same
 * store gives the same bytes on every run.  Same conventions as dmsa_hip.h (contexts, status codes, no CPU fallback).
 *
 * C1  PRECONDITIONS, else DMSA_ERR_INVALID with the reason in dmsa_last_error: everything N1 asks of `radius` (retention on, at least one
 *     retained row, voxel_size > 0, radius finite and in [voxel_size, 64 * voxel_size]); 1 <= min_size <= 2^26; max_size == 0 (no upper
 *     bound) or min_size <= max_size <= 2^26; retained rows <= 2^26.
 * C2  ADJACENT.  Rows i != j are adjacent iff d2 <= radius * radius, d2 being N2's float expression, operation for operation, and
 *     radius * radius the float product.  The relation is symmetric bit for bit (g_j - g_i is the exact negation of g_i - g_j, the squares
 *     are equal) and depends on no grid.
 * C3  CLUSTER.  The clusters are the connected components of the adjacency graph.  label_i = the smallest store row index in the cluster of
 *     row i (int32; label_i <= i, and label_i == i exactly once per cluster); size_i = the number of rows of that cluster (int32).  A row
 *     without an adjacent row is a cluster of size 1.
 * C4  KEEP.  Row i is kept iff size_i >= min_size and (max_size == 0 or size_i <= max_size).
 * C5  STATISTICS, all integers (any split of the sums gives the same values): rows, clusters, largest (the largest size); kept_rows,
 *     kept_clusters; small_rows (dropped by min_size), large_rows (dropped by max_size); rows = kept_rows + small_rows + large_rows.
 * C6  THE STORE, as O6.  Labels and a classification stay valid until a scan is added or the store is compacted by any stage.
 *     dmsa_dense_cloud_remove_clusters compacts the retained points (the fourth float included: an intensity travels, I-rules) and their
 *     origins to the kept rows, stably, in store order; the labels, the search grid, any normals and the other stages' classifications are
 *     then invalid.  The voxel set and dmsa_dense_stats are not touched.
 * C7  FILE.  A binary PCD of the store with its labels, rows in store order: `x y z label`, SIZE 4 4 4 4, TYPE F F F U, 16-byte rows; on an
 *     intensity object `x y z intensity label`, TYPE F F F F U, 20-byte rows.  The header is decided here (dmsa_pcd_header_xyz_label_binary),
 *     the counts twelve digits wide like the other headers.  The file needs labels of the store as it stands, else DMSA_ERR_INVALID; an
 *     empty store or a path that cannot be written leaves no partial file.
 */
#ifndef DMSA_DENSE_CLUSTERS_H
#define DMSA_DENSE_CLUSTERS_H

#include "dmsa_dense_outliers.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmsa_dense_cluster_config {
    float   radius;    /* 0.3: metres; two rows at most this far apart are adjacent (C2)                              */
    int32_t min_size;  /* 50:  clusters of fewer rows are dropped, 1 .. 2^26 (from no recorded data: a placeholder)   */
    int32_t max_size;  /* 0:   no upper bound; otherwise clusters of more rows are dropped, min_size .. 2^26          */
    int32_t pad;
} dmsa_dense_cluster_config;
void dmsa_default_dense_cluster_config(dmsa_dense_cluster_config* cfg);

typedef struct dmsa_dense_cluster_stats {
    int64_t rows, clusters, largest;
    int64_t kept_rows, kept_clusters;
    int64_t small_rows, large_rows; /* rows = kept_rows + small_rows + large_rows */
} dmsa_dense_cluster_stats;

/* The stage call of C2-C3 over all retained rows (of cfg only `radius` is read, min_size and max_size must still satisfy C1): label_out
 * and size_out, `rows` int32 each, either may be NULL.  The labels stay in HBM for dmsa_dense_cloud_save_pcd_labels. */
int dmsa_dense_cloud_cluster_labels(dmsa_dense_cloud* dc, const dmsa_dense_cluster_config* cfg, int32_t* label_out, int32_t* size_out);
/* C2-C5 for every retained row.  keep_out (rows bytes, 1 = kept, 0 = dropped) and stats may be NULL; the flags stay in HBM for
 * dmsa_dense_cloud_remove_clusters, independent of the other stages' classifications. */
int dmsa_dense_cloud_classify_clusters(dmsa_dense_cloud* dc, const dmsa_dense_cluster_config* cfg, uint8_t* keep_out, dmsa_dense_cluster_stats* stats);
/* C6.  Needs a classification that is still valid (none yet, a scan added since, or the store compacted since: DMSA_ERR_INVALID).
 * *kept (optional) = rows left in the store. */
int dmsa_dense_cloud_remove_clusters(dmsa_dense_cloud* dc, int64_t* kept);
/* C7.  *points_out / *bytes_out (optional) = rows in the file / its size. */
int dmsa_dense_cloud_save_pcd_labels(dmsa_dense_cloud* dc, const char* path, int64_t* points_out, int64_t* bytes_out);
/* Host only, no context: the header of C7 with width = n, `intensity` != 0 for the five-field layout; writes at most cap bytes incl. the
 * terminating 0; returns the length or a negative status. */
int dmsa_pcd_header_xyz_label_binary(int64_t n, int32_t intensity, char* out, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* DMSA_DENSE_CLUSTERS_H */
