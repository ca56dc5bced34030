/*
 * dmsa_dense_occupancy.h — C ABI of the occupancy map of the dense cloud (include/dmsa_dense_cloud.h): for every cell of a grid, whether the
 * measured rays saw it OCCUPIED, saw it FREE, or never observed it.  The retained store (include/dmsa_dense_normals.h, N0) keeps the sensor
 * origin o_i beside every survivor g_i: each pair is a measured ray.  The ray ended in the cell of g_i (a hit) and went through every cell
 * before it (a pass).  Carving (include/dmsa_dense_carve.h) walks the same rays to ask which POINTS other rays saw through; this header keeps
 * what the walk establishes about the SPACE, as a 3-D voxel file and as the 2-D map.pgm + map.yaml pair of the ROS map_server.
 *
 * Only the rays of the rows still in the store are evidence: the voxel thinning and every removal (O6, T7, C6, D6) take their rays with them.
 *
 * Like the rules 1-7, N0-N5, O1-O6 and T1-T7 the semantics are DECIDED HERE, stated below, and tested against an independent numpy model
 * (tests/dense_occupancy_model.py) bit for bit.  They are exact and order-free: integer counters, the integer walk of T3-T4, integer
 * comparisons.  No float is summed anywhere.  Same conventions as dmsa_hip.h (contexts, status codes, no CPU fallback).
 *
 * M1  PRECONDITIONS, else DMSA_ERR_INVALID with the reason in dmsa_last_error: retention on, at least one retained row, voxel_size > 0;
 *     retained rows <= 2^26; cell_size finite and in [voxel_size, 64 * voxel_size] (exactly T1's bound); max_length finite and > 0;
 *     1 <= min_hits <= 2^20; 1 <= min_passes <= 2^20; 1 <= occ_num <= 2^20; 1 <= occ_den <= 2^20; initial_slots is 0 (automatic) or a
 *     power of two in [64, 2^31].
 * M2  RAYS.  Row r is the ray o_r -> g_r.  Its length and the three cases in which it is SKIPPED are exactly T2's, with this config's
 *     max_length.  A skipped ray contributes nothing and is counted in rays_skipped.
 * M3  EVIDENCE.  The traversed cells of a ray are T4's, with c = (double)cell_size.  The LAST one, the endpoint's, gets hits += 1; every
 *     other traversed cell, the origin's included, gets passes += 1.  A ray that stays in one cell gives one hit and no pass.  A traversed
 *     cell outside [-2^20, 2^20) on some axis is not recorded: it is counted in cells_out_of_range (and in cells_traversed, like every
 *     traversed cell).  Both counters are uint32; with at most 2^26 rays neither can wrap.  Integer addition is associative: any split over
 *     lanes, waves and atomics gives the same counts, and the same bytes on every run.
 * M4  THE MAP is the set of cells with hits + passes > 0, LISTED in ascending order of the cell key
 *     (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20), the key of the search grid.  The listing is a function of the store and the config
 *     alone: it does not depend on the slot order of the table the counts were gathered in, nor on how often that table was rebuilt.
 * M5  STATE of a cell, integer comparisons with the products in uint64:
 *       OCCUPIED (2)  iff  hits >= min_hits  and  passes * occ_den <= hits * occ_num;
 *       else FREE (1) iff  passes >= min_passes;
 *       else UNKNOWN (0): the evidence is weak.
 *     A cell that is not in the map is unknown as well.  This is the clamp-free, order-free form of a log-odds update with a fixed weight per
 *     hit against a fixed weight per pass; the clamping that makes an octree map depend on the order of insertion is deliberately absent.
 * M6  THE VOXEL FILE is a binary PCD with rows of 24 bytes and six fields: x y z (F4), hits passes state (U4).  One row per map cell whose
 *     state is >= the caller's min_state (0, 1 or 2), in M4's order.  The coordinate of a cell on axis a is its centre,
 *     (float)(((double)c_a + 0.5) * (double)cell_size): one rounding, to float.  A file of zero rows is legal: the header alone.
 * M7  THE 2-D MAP.  Inputs z_lo <= z_hi, both finite.  With c = (double)cell_size the slab is the cells with
 *     floor((double)z_lo / c) <= cz <= floor((double)z_hi / c).  A COLUMN is a pair (cx, cy) for which some map cell lies in the slab.  The
 *     image covers the bounding box of the columns: width = cx_max - cx_min + 1, height = cy_max - cy_min + 1.  No column, or
 *     width * height > 2^28: DMSA_ERR_INVALID.  Pixel (col, row) is the column (cx_min + col, cy_max - row): image row 0 is the largest y.
 *     Its value is 0 if any slab cell of the column is OCCUPIED; otherwise 254 if any is FREE; otherwise 205 (columns with UNKNOWN cells
 *     only, and pairs of the box that are no column).  The PGM is "P5\n<width> <height>\n255\n" and the bytes, row by row.  The YAML is
 *     exactly six lines: "image: <basename of the pgm path>", "resolution: %.9g" of c, "origin: [%.9g, %.9g, 0]" of (cx_min * c, cy_min * c)
 *     computed in double, "negate: 0", "occupied_thresh: 0.65", "free_thresh: 0.196".  The basename is what follows the last '/'.
 * M8  VALIDITY.  A built map stays valid until a scan is added or the store is compacted by any stage, as T7 has it for a classification.
 *     Building it invalidates nothing: store, normals and every classification stay as they are (the search grid over the store is a cache
 *     that is rebuilt for the edge a call asks for; no result depends on it).  Every read or write call on a missing or stale map returns
 *     DMSA_ERR_INVALID.  A build that M1 refuses changes nothing, an earlier map included; a build that fails later leaves no map.
 *
 * THE TABLE the counts are gathered in is open addressing over {key, hits, passes}; a build that finds it more than half full doubles it and
 * walks all rays again (counts are additive from zero, so the second walk is exact).  The automatic first size is the smallest power of two
 * >= 4 * rows, at least 1024.  Past 2^31 slots the build returns DMSA_ERR_NOMEM, as the voxel table does.  initial_slots exists so that a
 * test can force rebuilds; table_slots and table_builds report what happened and are no part of the semantics.
 *
 * THE DEFAULTS come from a synthetic toy scene, not from recorded data.  A plane seen at a grazing angle is passed
 * through by the rays that land further along it -- at 6 degrees and cells of 0.2 m about ten passes per hit -- so occ_num / occ_den sits
 * well above 1.
 */
#ifndef DMSA_DENSE_OCCUPANCY_H
#define DMSA_DENSE_OCCUPANCY_H

#include "dmsa_dense_carve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DMSA_OCCUPANCY_UNKNOWN 0
#define DMSA_OCCUPANCY_FREE 1
#define DMSA_OCCUPANCY_OCCUPIED 2

typedef struct dmsa_dense_occupancy_config {
    float   cell_size;      /* 0.2: metres; edge of the cells (T3)                                          */
    float   max_length;     /* 30:  metres; longer rays are skipped (T2)                                    */
    int32_t min_hits;       /* 1:   hits a cell needs to be called occupied, 1 .. 2^20                      */
    int32_t min_passes;     /* 2:   passes a cell needs to be called free, 1 .. 2^20                        */
    int32_t occ_num;        /* 16:  occupied iff passes * occ_den <= hits * occ_num; each 1 .. 2^20         */
    int32_t occ_den;        /* 1                                                                            */
    int64_t initial_slots;  /* 0:   automatic; else the first table size, a power of two in [64, 2^31]      */
    /* (six 4-byte fields before the 8-byte one: 32 bytes, and no room for implicit padding) */
} dmsa_dense_occupancy_config;
void dmsa_default_dense_occupancy_config(dmsa_dense_occupancy_config* cfg);

typedef struct dmsa_dense_occupancy_stats {
    int64_t rows, rays_walked, rays_skipped;    /* rows = rays_walked + rays_skipped                        */
    int64_t cells_traversed, cells_out_of_range; /* summed over the walked rays                             */
    int64_t cells, occupied, free, unknown;     /* the map: cells = occupied + free + unknown               */
    int64_t table_slots, table_builds;          /* of the last build; builds > 1: the table was doubled     */
} dmsa_dense_occupancy_stats;

typedef struct dmsa_dense_occupancy_slice_info {
    int32_t width, height, cx_min, cy_min;
    double  origin_x, origin_y;                 /* cx_min * c, cy_min * c                                   */
    int64_t occupied, free, unknown;            /* pixels of value 0, 254, 205: their sum is width * height */
} dmsa_dense_occupancy_slice_info;

/* Host only, no context: M5.  0, 1 or 2; DMSA_ERR_INVALID (negative) for a NULL config or one whose min_hits, min_passes, occ_num or occ_den
 * M1 refuses (the other fields are not looked at). */
int dmsa_dense_occupancy_state(const dmsa_dense_occupancy_config* cfg, uint32_t hits, uint32_t passes);
/* Host only: the header of M6's file for n rows, as dmsa_pcd_header_xyz_binary: its length, or DMSA_ERR_INVALID. */
int dmsa_pcd_header_occupancy_binary(int64_t n, char* out, int32_t cap);
/* Host only: M7's texts, their length or DMSA_ERR_INVALID (a NULL or short buffer, a size < 1, a cell_size that is not finite or not > 0). */
int dmsa_occupancy_map_pgm_header(int32_t width, int32_t height, char* out, int32_t cap);
int dmsa_occupancy_map_yaml(const char* pgm_path, float cell_size, int32_t cx_min, int32_t cy_min, char* out, int32_t cap);

/* M2-M5 for every retained row.  The map stays in HBM.  stats may be NULL. */
int dmsa_dense_cloud_build_occupancy(dmsa_dense_cloud* dc, const dmsa_dense_occupancy_config* cfg, dmsa_dense_occupancy_stats* stats);
/* The cells [first, first + count) of M4's listing: cells_xyz (3 int32 each), hits, passes (uint32), state (uint8).  Any output may be NULL;
 * *total (optional) = cells of the map.  A window beyond the listing: DMSA_ERR_INVALID. */
int dmsa_dense_cloud_occupancy_cells(dmsa_dense_cloud* dc, int64_t first, int64_t count, int32_t* cells_xyz, uint32_t* hits, uint32_t* passes, uint8_t* state,
                                     int64_t* total);
/* M6.  min_state outside 0 .. 2: DMSA_ERR_INVALID.  *rows_written is optional.  A failure leaves no partial file. */
int dmsa_dense_cloud_save_pcd_occupancy(dmsa_dense_cloud* dc, const char* path, int32_t min_state, int64_t* rows_written);
/* M7.  info is filled whenever the slab has a column and the image is not too large; the width * height bytes go to pixels (may be NULL: the
 * size alone) when cap holds them, DMSA_ERR_INVALID otherwise. */
int dmsa_dense_cloud_occupancy_slice(dmsa_dense_cloud* dc, float z_lo, float z_hi, dmsa_dense_occupancy_slice_info* info, uint8_t* pixels, int64_t cap);
/* M7's two files.  A failure leaves neither. */
int dmsa_dense_cloud_save_occupancy_map(dmsa_dense_cloud* dc, const char* pgm_path, const char* yaml_path, float z_lo, float z_hi);

#ifdef __cplusplus
}
#endif
#endif /* DMSA_DENSE_OCCUPANCY_H */
