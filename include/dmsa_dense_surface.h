/*
 * dmsa_dense_surface.h — C ABI of the fused surface of the dense cloud (include/dmsa_dense_cloud.h): a truncated signed distance field (TSDF)
 * summed from the measured rays, as a voxel file, and its zero set as a triangle mesh.  The retained store (include/dmsa_dense_normals.h, N0)
 * keeps the sensor origin o_r beside every survivor g_r: each pair is a measured ray.  The occupancy map (include/dmsa_dense_occupancy.h) keeps
 * what the rays say about each cell as two counters; this header keeps HOW FAR in front of or behind the measured surface each cell near an
 * endpoint lies, averaged over all rays that cross it, and triangulates where that average changes sign.
 *
 * Only the rays of the rows still in the store are evidence: the voxel thinning and every removal (O6, T7, C6, D6) take their rays with them.
 *
 * Like the rules M1-M8 the semantics are DECIDED HERE, stated below, and tested against an independent numpy model
 * (tests/dense_surface_model.py) bit for bit.  The fusion is exact and order-free: every ray contributes integers, and integers are summed.
 * Same conventions as dmsa_hip.h (contexts, status codes, no CPU fallback).
 *
 * S1  PRECONDITIONS, else DMSA_ERR_INVALID with the reason in dmsa_last_error: retention on, at least one retained row, voxel_size > 0;
 *     retained rows <= 2^26; cell_size finite and in [voxel_size, 64 * voxel_size] (T1's bound); truncation finite and in
 *     [cell_size, 16 * cell_size]; max_length finite and > 0; 1 <= min_weight <= 2^20; initial_slots is 0 (automatic) or a power of two in
 *     [64, 2^31].
 * S2  RAYS.  Row r is the ray o_r -> g_r; d, L2 and L are exactly T2's.  The ray is skipped if L2 == 0 or L > max_length.
 * S3  THE INTEGRATED SEGMENT, in float, each operation rounded on its own: f = truncation / L; per axis p_a = f * d_a, b_a = g_a + p_a, and
 *     a_a = g_a - p_a if L > truncation, else a_a = o_a.  The segment a -> b is walked with T3 / T4 at c = (double)cell_size; a segment that
 *     T2's third case refuses (an end beyond 2^31 cells, end cells more than 2^11 apart on an axis) skips the ray as well.  A skipped ray is
 *     counted in rays_skipped and contributes nothing.
 * S4  A SAMPLE.  For every traversed cell (cx, cy, cz) inside [-2^20, 2^20)^3 (the others are counted in cells_out_of_range, and in
 *     cells_traversed like every traversed cell): the centre m_a = (float)(((double)c_a + 0.5) * c), M6's; in float u = g - m per axis;
 *     s = u_x * d_x; s += u_y * d_y; s += u_z * d_z; s = s / L; s = fminf(fmaxf(s, -truncation), truncation);
 *     q = (int32) rintf((s / truncation) * 32768.0f), so q lies in [-32768, 32768].  Positive: in front of the surface, on the sensor's side.
 * S5  FUSION.  A cell keeps sum (int64, the sum of its q) and n (uint32, its samples).  Both are integer additions: any split over lanes,
 *     waves and atomics gives the same values, and the same bytes on every run.  2^26 * 2^15 < 2^63 and n <= 2^26: neither can wrap.
 * S6  THE VOLUME is the set of cells with n > 0, LISTED in ascending order of M4's cell key.  The listing is a function of the store and the
 *     config alone: it does not depend on the slot order of the table the sums were gathered in, nor on how often that table was rebuilt.
 * S7  THE VOXEL FILE is a binary PCD with rows of 20 bytes and five fields: x y z tsdf (F4) weight (U4), one row per cell in S6's order.
 *     x y z is S4's centre; tsdf = (float)(((double)sum / (double)n) / 32768.0 * (double)truncation); weight = n.
 * S8  THE MESH: marching tetrahedra on the lattice of the cell centres.  A node (a listed cell) is VALID iff n >= min_weight and INSIDE iff
 *     it is valid and sum < 0 (sum == 0 is outside).  Every valid node is the ANCHOR of a cube whose corners are the nodes at the offsets
 *     (m & 1, m >> 1 & 1, m >> 2 & 1) for the corner masks m = 0 .. 7.  The cube is cut into the six Kuhn tetrahedra
 *     {0, 1 << a, (1 << a) | (1 << b), 7}, the permutations (a, b, c) taken in the order xyz, xzy, yxz, yzx, zxy, zyx: the cut matches on
 *     shared faces, so the surface is watertight wherever the volume is.  A tetrahedron is MESHED iff all four of its nodes are valid.
 *     One or three inside corners give one triangle, two give two, none or four give none.
 *     VERTICES lie on edges between two corners whose masks are nested, p inside q: the lower node is anchor + offset(p), the CLASS of the
 *     edge is q & ~p (1 .. 7), and the vertex is identified by (listing index of its lower node, class): every triangle that touches it
 *     shares it.  With m0 = (double)sum0 / (double)n0 at the lower node and m1 at the upper, t = m0 / (m0 - m1) in double and
 *     pos_a = (float)((((double)c0_a + 0.5) + t * (double)off_a) * c), off = offset(class).
 *     CORNER ORDER of a triangle, with the tetrahedron's chain v0 .. v3 (ascending masks): one inside corner A: the crossings on A's three
 *     edges in chain order of the other end; three inside corners: the same around the single outside corner; two inside corners A < B
 *     and outside C < D: the quad AC, AD, BD, BC split into (AC, AD, BD) and (AC, BD, BC).
 *     ORIENTATION: the last two corners are swapped where needed so that the normal N = (v1 - v0) x (v2 - v0) points to the outside, the side
 *     the sensor stood on.  That depends on the (tetrahedron, inside set) case alone and is derived in integers, in doubled lattice
 *     coordinates with the crossings at the edge midpoints: N dotted with (centroid of the outside corners - centroid of the inside ones)
 *     is positive (it is never zero).
 *     A vertex EXISTS iff a triangle refers to it.  Vertices are ordered by (lower node's listing index, class), triangles by (anchor's listing
 *     index, tetrahedron 0 .. 5, triangle 0 .. 1).  Degenerate triangles (a crossing at t = 0 or 1) are kept.  More than 2^31 - 1 vertices or
 *     triangles: DMSA_ERR_INVALID.
 * S9  THE MESH FILE is a binary little-endian PLY: "ply\nformat binary_little_endian 1.0\nelement vertex V\nproperty float x\nproperty float y\n
 *     property float z\nelement face F\nproperty list uchar int vertex_indices\nend_header\n", then V rows of 12 bytes and F rows of 13 bytes
 *     (the byte 3 and three int32).  A mesh without a triangle is a legal file: the header alone.  A failure leaves no partial file.
 * S10 VALIDITY is M8's.  A built volume stays valid until a scan is added or the store is compacted by any stage; building it invalidates
 *     nothing else (store, normals, every classification and the occupancy map stay as they are).  The mesh is derived from the volume: it is
 *     valid while the volume it was extracted from is, and an extraction with another min_weight replaces it.  Every read or write call on a
 *     missing or stale volume or mesh returns DMSA_ERR_INVALID.  A build that S1 refuses changes nothing; a build that fails later leaves
 *     neither volume nor mesh; a new build leaves no mesh.
 *
 * THE TABLE the sums are gathered in follows the occupancy map's policy: open addressing, doubled and walked again when more than half full
 * (exact, since the sums start from zero), the automatic first size the smallest power of two >= 4 * rows and at least 1024, DMSA_ERR_NOMEM
 * past 2^31 slots.  table_slots and table_builds report what happened and are no part of the semantics.
 *
 * THE DEFAULTS are placeholders from a synthetic toy scene, not from recorded data.
 */
#ifndef DMSA_DENSE_SURFACE_H
#define DMSA_DENSE_SURFACE_H

#include "dmsa_dense_occupancy.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmsa_dense_surface_config {
    float   cell_size;      /* 0.2: metres; edge of the cells (T3)                                          */
    float   truncation;     /* 0.6: metres; the field is cut off at this distance, cell_size .. 16 cells    */
    float   max_length;     /* 30:  metres; longer rays are skipped (T2)                                    */
    int32_t min_weight;     /* 2:   samples a cell needs to count (cells_valid; the default of a mesh)      */
    int64_t initial_slots;  /* 0:   automatic; else the first table size, a power of two in [64, 2^31]      */
    /* (four 4-byte fields before the 8-byte one: 24 bytes, and no room for implicit padding) */
} dmsa_dense_surface_config;
void dmsa_default_dense_surface_config(dmsa_dense_surface_config* cfg);

typedef struct dmsa_dense_surface_stats {
    int64_t rows, rays_walked, rays_skipped;      /* rows = rays_walked + rays_skipped                       */
    int64_t cells_traversed, cells_out_of_range;  /* summed over the walked rays                             */
    int64_t cells, cells_valid;                   /* the volume; those with n >= the config's min_weight     */
    int64_t table_slots, table_builds;            /* of the last build; builds > 1: the table was doubled    */
} dmsa_dense_surface_stats;

typedef struct dmsa_dense_mesh_stats {
    int64_t tetrahedra_meshed, vertices, triangles;
} dmsa_dense_mesh_stats;

/* Host only, no context: S2-S4 for the ray o -> g (3 floats each) through the header the device kernels compile.  *n = -1 for a skipped ray,
 * else the samples (the traversed cells inside the range, in walk order): the first min(*n, cap) of them go to cells_xyz (3 int32 each) and
 * q.  cap 0 counts.  DMSA_ERR_INVALID for a NULL argument or a config that S1 refuses on its own (cell_size is only asked to be finite and
 * > 0 here: the voxel is the store's). */
int dmsa_dense_surface_samples(const dmsa_dense_surface_config* cfg, const float* o, const float* g, int32_t* cells_xyz, int32_t* q, int64_t cap, int64_t* n);
/* Host only: the header of S7's file for n rows, as dmsa_pcd_header_xyz_binary: its length, or DMSA_ERR_INVALID. */
int dmsa_pcd_header_tsdf_binary(int64_t n, char* out, int32_t cap);
/* Host only: the header of S9's file: its length, or DMSA_ERR_INVALID (a count outside [0, 2^31 - 1], a NULL or short buffer). */
int dmsa_ply_header_mesh(int64_t vertices, int64_t triangles, char* out, int32_t cap);

/* S2-S6 for every retained row.  The volume stays in HBM.  stats may be NULL. */
int dmsa_dense_cloud_build_surface(dmsa_dense_cloud* dc, const dmsa_dense_surface_config* cfg, dmsa_dense_surface_stats* stats);
/* The cells [first, first + count) of S6's listing: cells_xyz (3 int32 each), sum (int64), n (uint32).  Any output may be NULL; *total
 * (optional) = cells of the volume.  A window beyond the listing: DMSA_ERR_INVALID. */
int dmsa_dense_cloud_surface_cells(dmsa_dense_cloud* dc, int64_t first, int64_t count, int32_t* cells_xyz, int64_t* sum, uint32_t* n, int64_t* total);
/* S7.  *rows_written is optional.  A failure leaves no partial file. */
int dmsa_dense_cloud_save_pcd_tsdf(dmsa_dense_cloud* dc, const char* path, int64_t* rows_written);
/* S8 of the built volume.  min_weight outside [1, 2^20]: DMSA_ERR_INVALID.  The mesh stays in HBM.  stats may be NULL. */
int dmsa_dense_cloud_extract_mesh(dmsa_dense_cloud* dc, int32_t min_weight, dmsa_dense_mesh_stats* stats);
/* The vertices [first, first + count) (3 floats each) and the triangles [first, first + count) (3 int32 each) of the extracted mesh.  The
 * output may be NULL; *total (optional) = all of them.  A window beyond the end: DMSA_ERR_INVALID. */
int dmsa_dense_cloud_mesh_vertices(dmsa_dense_cloud* dc, int64_t first, int64_t count, float* xyz, int64_t* total);
int dmsa_dense_cloud_mesh_triangles(dmsa_dense_cloud* dc, int64_t first, int64_t count, int32_t* indices, int64_t* total);
/* S9.  A failure leaves no partial file. */
int dmsa_dense_cloud_save_ply_mesh(dmsa_dense_cloud* dc, const char* path);

#ifdef __cplusplus
}
#endif
#endif /* DMSA_DENSE_SURFACE_H */
