/*
 * dmsa_dense_compare.h — C ABI of the comparison of the dense cloud (include/dmsa_dense_cloud.h) with a REFERENCE CLOUD: for every
 * retained row (include/dmsa_dense_normals.h, N0) the nearest reference point, for every reference point the nearest retained row, exact
 * statistics of both sets of distances, the store compacted to what the reference confirms (or to what changed), and the store written
 * with its distances.  What CloudCompare's "cloud / cloud distance" does against a surveyed ground-truth cloud or the map of another run,
 * on the points where they already are.
 *
 * Like O1-O6, T1-T7 and C1-C7 the semantics are DECIDED HERE, stated below, and tested against an independent model
 * (tests/dense_compare_model.py).  They are chosen so that the result does not depend on how lanes, waves, tiles or atomics interleave:
 * the same inputs give the same bytes on every run.  Same conventions as dmsa_hip.h (contexts, status codes, no CPU fallback).  An object
 * that never sets a reference allocates and launches what it did before.
 *
 * D0  THE REFERENCE.  dmsa_dense_cloud_set_reference uploads n <= 2^26 host rows of stride_floats >= 3 floats once; T == NULL is the
 *     identity, otherwise T is a row-major 3 x 4 rigid alignment into the map frame: its twelve doubles are cast to float and every row is
 *     transformed on the device in rule 5's form, ((c0*x + c1*y) + c2*z) + c3 per output row, each operation rounded on its own.  A
 *     reference row is VALID iff its three (transformed) coordinates are finite and pass rule 6's grid bound at the object's voxel_size:
 *     floorf(c / voxel_size) in [-2^20, 2^20) on every axis (voxel_size <= 0: DMSA_ERR_INVALID).  An invalid row keeps its row number; it is
 *     never a candidate and never a query and is counted in ref_invalid.  The reference is not thinned; duplicate points are legal.  It
 *     belongs to the object, not to the store: it survives added scans and compactions (only results that depend on the store go stale).
 *     A new call replaces it; n == 0 drops it.
 * D1  PRECONDITIONS of the calls below, else DMSA_ERR_INVALID with the reason in dmsa_last_error: everything N1 asks, of `max_distance`
 *     in the place of `radius` (retention on, at least one retained row, voxel_size > 0, max_distance finite and in
 *     [voxel_size, 64 * voxel_size]); a reference with at least one valid row; tolerance finite, 0 < tolerance <= max_distance; retained
 *     rows <= 2^26.
 * D2  NEAREST of a query point q in a set S.  The candidates are the rows s of S with d2 <= max_distance * max_distance (the float
 *     product), d2 being N2's float expression with d = s - q, operation for operation.  The nearest row minimises the pair
 *     (d2, row index in S) lexicographically: equal distances go to the smallest row index.  A minimum over such pairs is associative and
 *     commutative, and a non-negative float orders as its bit pattern, so (bits(d2) << 32) | row is one 64-bit key and ANY split of the
 *     candidates gives the same winner.  dist = sqrtf(d2_min), correctly rounded.  No candidate: the query is UNMATCHED, dist is a quiet
 *     NaN (0x7FC00000) and index = -1.
 * D3  TWO DIRECTIONS, each a stage call over a row range.  ACCURACY (dmsa_dense_cloud_nearest_in_reference): the queries are store rows,
 *     S the valid reference rows, the indices reference row numbers as the caller passed them.  COMPLETENESS
 *     (dmsa_dense_cloud_nearest_in_store): the queries are the valid reference rows, S the store rows; an invalid reference row reports NaN
 *     and -1 and is NOT counted as unmatched.
 * D4  EXACT STATISTICS per direction.  The scale of O4: frexpf(max_distance) = m * 2^e, scale = 2^(18 - e).  q_i = (int64)rintf(dist_i *
 *     scale): the product is exact, and q_i <= 2^18 (sqrtf of a d2 no larger than the float square of max_distance is no larger than
 *     max_distance: O4's argument).  Over the matched queries int64 matched, S1 = sum q_i, S2 = sum q_i^2; int64 unmatched; int64 within =
 *     the matched queries with d2 <= tolerance * tolerance (the float product); a histogram of 64 int64 bins, bin = min(q_i >> 12, 63), a
 *     bin 2^(e - 6) metres wide.  All are integer sums: any split gives the same values.
 * D5  SUMMARY, on the host, in double, each operation rounded on its own (dmsa_dense_compare_summary): mean = S1 / matched / scale;
 *     rms = sqrt(S2 / matched) / scale; fraction_within = within / queries.  precision = the accuracy direction's fraction (queries = rows),
 *     recall = the completeness direction's (queries = valid reference rows), f_score = 2 * precision * recall / (precision + recall).
 *     Every quotient with a zero denominator is 0.
 * D6  CLASSIFY AND REMOVE, the store only.  DMSA_COMPARE_KEEP_NEAR: row i is kept iff it is matched and d2 <= tolerance^2 (what the
 *     reference confirms); DMSA_COMPARE_KEEP_FAR: the complement (what changed).  dmsa_dense_cloud_remove_by_reference compacts points
 *     (the fourth float included) and origins to the kept rows as O6 / C6 do, by a classification of this stage's own; the voxel set and
 *     dmsa_dense_stats are not touched.  Afterwards this stage's distances and classification are stale like the grid, the normals, the
 *     labels and the other classifications; the reference is not.
 * D7  FILE.  A binary PCD of the store with its ACCURACY distances, rows in store order: `x y z distance`, TYPE F F F F, 16-byte rows; on
 *     an intensity object `x y z intensity distance`, 20-byte rows; unmatched rows carry the quiet NaN.  The header is decided here
 *     (dmsa_pcd_header_xyz_distance_binary), the counts twelve digits wide.  The file needs distances of the store as it stands against the
 *     reference as it stands (dmsa_dense_cloud_compare or classify_by_reference since either changed), else DMSA_ERR_INVALID; no partial
 *     file on failure.
 * D8  A REFERENCE FROM A FILE, host only, no context.  Accepted: PCD v0.7, DATA binary, fields x, y and z among the FIELDS in any position,
 *     each SIZE 4, TYPE F, COUNT 1; any other field of any SIZE x COUNT is skipped by stride; WIDTH x HEIGHT == POINTS, zero-padded or not;
 *     a file long enough for the rows.  That is every file this library writes.  Anything else (ascii, binary_compressed, a missing or
 *     mistyped coordinate field, a short file, a count that overflows, a header line longer than the buffer) gives DMSA_ERR_INVALID, the
 *     reason naming what was met (dmsa_pcd_xyz_last_error, per thread), and nothing is written.
 */
#ifndef DMSA_DENSE_COMPARE_H
#define DMSA_DENSE_COMPARE_H

#include "dmsa_dense_clusters.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DMSA_COMPARE_KEEP_NEAR 0
#define DMSA_COMPARE_KEEP_FAR 1
#define DMSA_COMPARE_BINS 64

typedef struct dmsa_dense_compare_config {
    float   max_distance;  /* 1.0: metres; the reach of the search (D2).  Ten voxels of the demo's 0.1 m: from no recorded data, a placeholder */
    float   tolerance;     /* 0.1: metres; `within`, precision / recall and D6.  One voxel of the demo: a placeholder as well                  */
    int32_t keep;          /* DMSA_COMPARE_KEEP_NEAR; read by classify_by_reference only                                                      */
    int32_t pad;
} dmsa_dense_compare_config;
void dmsa_default_dense_compare_config(dmsa_dense_compare_config* cfg);

/* D4 and D5 of one direction; queries = matched + unmatched */
typedef struct dmsa_dense_compare_direction {
    int64_t queries, matched, unmatched, within, s1, s2;
    int64_t histogram[DMSA_COMPARE_BINS];
    double  mean_m, rms_m, fraction_within;
} dmsa_dense_compare_direction;

typedef struct dmsa_dense_compare_stats {
    int64_t rows, ref_rows, ref_invalid; /* store rows; reference rows, the invalid ones included; of those the invalid */
    int64_t kept;                        /* classify_by_reference: rows kept; compare: 0                                */
    double  scale, bin_width_m;          /* D4: 2^(18 - e) and 2^(e - 6)                                                */
    dmsa_dense_compare_direction accuracy, completeness; /* classify_by_reference fills `accuracy` only                */
    double  precision, recall, f_score;  /* D5                                                                          */
} dmsa_dense_compare_stats;

/* D0. */
int dmsa_dense_cloud_set_reference(dmsa_dense_cloud* dc, const float* xyz, int64_t n, int32_t stride_floats, const double* T);
/* Rows [first, first + count) of the reference as transformed: xyz_out (count x 3 floats) and valid_out (count bytes), either may be NULL;
 * *total_out (optional) = reference rows.  Rows beyond the reference: DMSA_ERR_INVALID (with *total_out set). */
int dmsa_dense_cloud_reference(dmsa_dense_cloud* dc, int64_t first, int64_t count, float* xyz_out, uint8_t* valid_out, int64_t* total_out);

/* D2-D3, the stage calls: dist_out / index_out (count each, either may be NULL) of store rows [first, first + count) against the
 * reference, and of reference rows [first, first + count) against the store.  Of cfg, `keep` is not read. */
int dmsa_dense_cloud_nearest_in_reference(dmsa_dense_cloud* dc, const dmsa_dense_compare_config* cfg, int64_t first, int64_t count, float* dist_out, int32_t* index_out);
int dmsa_dense_cloud_nearest_in_store(dmsa_dense_cloud* dc, const dmsa_dense_compare_config* cfg, int64_t first, int64_t count, float* dist_out, int32_t* index_out);
/* D2-D5, both directions over all rows.  The accuracy distances stay in HBM for dmsa_dense_cloud_save_pcd_distance. */
int dmsa_dense_cloud_compare(dmsa_dense_cloud* dc, const dmsa_dense_compare_config* cfg, dmsa_dense_compare_stats* stats);
/* Host only, no context: D5 of one direction.  Any of the three outputs may be NULL.  A negative count, or a scale that is not finite and
 * positive: DMSA_ERR_INVALID. */
int dmsa_dense_compare_summary(int64_t matched, int64_t s1, int64_t s2, int64_t within, int64_t queries, double scale, double* mean_m, double* rms_m,
                               double* fraction_within);
/* D6.  keep_out (rows bytes, 1 = kept) and stats may be NULL; the flags stay in HBM for dmsa_dense_cloud_remove_by_reference. */
int dmsa_dense_cloud_classify_by_reference(dmsa_dense_cloud* dc, const dmsa_dense_compare_config* cfg, uint8_t* keep_out, dmsa_dense_compare_stats* stats);
int dmsa_dense_cloud_remove_by_reference(dmsa_dense_cloud* dc, int64_t* kept);
/* D7.  *points_out / *bytes_out (optional) = rows in the file / its size. */
int dmsa_dense_cloud_save_pcd_distance(dmsa_dense_cloud* dc, const char* path, int64_t* points_out, int64_t* bytes_out);
int dmsa_pcd_header_xyz_distance_binary(int64_t n, int32_t intensity, char* out, int32_t cap);
/* D8.  info: *points = the rows of the file.  read: the first min(cap, rows) rows into xyz_out (3 floats each), *points = the rows of the
 * file (cap < rows: DMSA_ERR_INVALID, nothing written, *points set).  The reason of a refusal: dmsa_pcd_xyz_last_error (this thread's last). */
int dmsa_pcd_xyz_info(const char* path, int64_t* points);
int dmsa_pcd_xyz_read(const char* path, float* xyz_out, int64_t cap, int64_t* points);
const char* dmsa_pcd_xyz_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DMSA_DENSE_COMPARE_H */
