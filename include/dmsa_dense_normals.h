/*
 * dmsa_dense_normals.h — C ABI of a normal and a curvature per point of the dense cloud (include/dmsa_dense_cloud.h): radius neighbourhoods
 * over ALL retained points, each normal turned toward the place where the sensor stood when its point was measured.
 *
 * Like the rules 1-7 of the dense cloud, the semantics are DECIDED HERE, stated below, and tested against an independent numpy model
 * (tests/dense_normals_model.py).  Same conventions as dmsa_hip.h (contexts, status codes, no CPU fallback).
 *
 * N0  RETENTION.  dmsa_dense_cloud_retain(dc) is legal only before the first scan is added (later: DMSA_ERR_INVALID).  From then on every
 *     survivor of rules 1-7 is also appended, in file order, to a store in HBM that grows by doubling: the point g and its SENSOR ORIGIN o
 *     = rule 5 applied to the sensor-frame point (0, 0, 0) with that point's own pose (the same apply_row3 order, the same floats).  32 bytes
 *     per point.  A call that is refused or rolled back (capacity too small, failed write, DMSA_ERR_NOMEM) leaves the store as it was, like
 *     the voxel table.  An object that does not retain does what it did: same bytes, same memory.
 * N1  PRECONDITIONS of the neighbourhood calls, else DMSA_ERR_INVALID with the reason in dmsa_last_error: retention on; at least one
 *     retained point; voxel_size > 0; radius finite; voxel_size <= radius <= 64 * voxel_size.  (At most 130^3 < 2^22 voxels meet a ball's
 *     bounding cube and one point survives per voxel: the integer sums of N3 cannot overflow.  radius >= voxel_size keeps the cells of the
 *     search grid inside the 21 bits per axis of the voxel grid.)
 * N2  NEIGHBOURHOOD of row i: every retained row j, i itself included, with d2 <= radius * radius, all in float, each operation rounded
 *     on its own: dx = g_j.x - g_i.x (dy, dz alike); d2 = dx*dx; d2 += dy*dy; d2 += dz*dz.  The set does not depend on any grid.
 * N3  MOMENTS, exact.  frexpf(radius) = m * 2^e; scale = 2^(20 - e).  Per neighbour and axis q_a = (int32)rintf(d_a * scale) (the product
 *     is exact, the rounding to nearest even).  Ten int64 sums: n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz.  Integer addition is
 *     associative: ANY split of the neighbour list over lanes, waves, tiles or atomics gives the same ten integers.
 * N4  NORMAL.  n < max(3, min_neighbours): four quiet NaNs.  Otherwise, in double without contraction,
 *     c_ab = ((double)S_ab - ((double)S_a * (double)S_b) / (double)n) / (double)n; the six values cast to float and NOT scaled back (eigen33
 *     rescales by the largest entry; normal and curvature are scale-free); then what dmsa_update_normals does from its covariance on
 *     (csrc/pcl_eigen33.h: pcl::computeRoots, the largest of the three cross products, curvature = |lambda_0 / trace|); the flip uses the
 *     per-point view vector w = o_i - g_i and wx*nx + wy*ny + wz*nz < 0.
 * N5  FILE.  A binary PCD with the header (decided here, self-describing; NOT "as PCL writes it")
 *       # .PCD v0.7 - Point Cloud Data file format | VERSION 0.7 | FIELDS x y z normal_x normal_y normal_z curvature | SIZE 4 4 4 4 4 4 4 |
 *       TYPE F F F F F F F | COUNT 1 1 1 1 1 1 1 | WIDTH <n> | HEIGHT 1 | VIEWPOINT 0 0 0 1 0 0 0 | POINTS <n> | DATA binary
 *     one line each, <n> twelve zero-padded digits as in the x y z file; rows of 28 bytes, compact, little-endian floats.
 */
#ifndef DMSA_DENSE_NORMALS_H
#define DMSA_DENSE_NORMALS_H

#include "dmsa_dense_cloud.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmsa_dense_normals_config {
    float   radius;          /* 0.3: metres                                                       */
    int32_t min_neighbours;  /* 5:   rows with fewer neighbours (itself included) get NaNs; >= 0  */
} dmsa_dense_normals_config;
void dmsa_default_dense_normals_config(dmsa_dense_normals_config* cfg);

/* N0 */
int dmsa_dense_cloud_retain(dmsa_dense_cloud* dc);
/* Rows [first, first + count) of the store: xyz_out / origin_out (count x 4 floats each, w = 1; either may be NULL), *total_out (optional) =
 * rows retained so far.  Rows beyond the store: DMSA_ERR_INVALID (with *total_out set). */
int dmsa_dense_cloud_retained(dmsa_dense_cloud* dc, int64_t first, int64_t count, float* xyz_out, float* origin_out, int64_t* total_out);

/* The stage call of N2-N3: the ten moments of rows [first, first + count), as the kernel behind dmsa_dense_cloud_compute_normals sums them. */
int dmsa_dense_cloud_neighbour_moments(dmsa_dense_cloud* dc, const dmsa_dense_normals_config* cfg, int64_t first, int64_t count,
                                       int64_t* moments /* count x 10 */);
/* N2-N4 for every retained row; the result stays in HBM for dmsa_dense_cloud_save_pcd_normals until the next scan is added.
 * normal_out: total x 4 floats (nx, ny, nz, curvature), may be NULL; *total (optional) = rows; *without_normal (optional) = rows with fewer than
 * max(3, min_neighbours) neighbours (a neighbourhood that has the rows but spans no plane -- all on a line -- gets what eigen33 gives it). */
int dmsa_dense_cloud_compute_normals(dmsa_dense_cloud* dc, const dmsa_dense_normals_config* cfg, float* normal_out, int64_t* total,
                                     int64_t* without_normal);
/* Host only, no context: N4 for one row.  view = o - g. */
int dmsa_dense_normal_from_moments(const int64_t m[10], const float view[3], int32_t min_neighbours, float out[4]);

/* N5.  The header call is host-only, with the arguments and the return of its x y z twin in dmsa_dense_cloud.h.  save needs a completed
 * dmsa_dense_cloud_compute_normals since the last added scan, else DMSA_ERR_INVALID; a path that cannot be written gives DMSA_ERR_INVALID
 * and leaves no partial file.  *points_out / *bytes_out (optional) = rows in the file / its size.  The streaming x y z file of
 * dmsa_dense_cloud_open_pcd / close_pcd is independent of all this. */
int dmsa_pcd_header_normals_binary(int64_t n, char* out, int32_t cap);
int dmsa_dense_cloud_save_pcd_normals(dmsa_dense_cloud* dc, const char* path, int64_t* points_out, int64_t* bytes_out);

#ifdef __cplusplus
}
#endif
#endif /* DMSA_DENSE_NORMALS_H */
