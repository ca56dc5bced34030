/*
 * dmsa_dense_carve.h — C ABI of the removal of moving objects from the dense cloud (include/dmsa_dense_cloud.h) by exact ray carving.  The
 * retained store (include/dmsa_dense_normals.h, N0) keeps the sensor origin o_i beside every survivor g_i: each pair is a measured ray, and
 * the space between its ends was seen empty at that moment.  A retained point that several other rays pass straight through was not there
 * when those rays were shot: it is TRANSIENT (a person, a car, a door), and the store is compacted to the rest.
 *
 * The test is per point, not per voxel, and its cone has its apex at the ray's ENDPOINT: a surface hit at grazing angle theta lies at
 * angle theta from the ray as seen from the endpoint, so with a cone half-angle below theta a ray cannot carve the surface it landed on.
 *
 * Like the rules 1-7, N0-N5 and O1-O6 the semantics are DECIDED HERE, stated below, and tested against an independent numpy model
 * (tests/dense_carve_model.py) bit for bit.  They are exact and order-free: integer counters, an integer grid walk, float predicates stated
 * operation for operation.  Same conventions as dmsa_hip.h (contexts, status codes, no CPU fallback).
 *
 * T1  PRECONDITIONS, else DMSA_ERR_INVALID with the reason in dmsa_last_error: retention on, at least one retained row, voxel_size > 0;
 *     cell_size finite and in [voxel_size, 64 * voxel_size] (this keeps cells inside 21 bits per axis, as N1 does); rho, end_margin,
 *     start_margin, max_length finite; rho > 0, end_margin > 0, start_margin >= 0, max_length > 0; 0 < tan_half_angle <= 1;
 *     1 <= min_passes <= 2^20; retained rows <= 2^26.
 * T2  RAYS.  Row r is a ray from o_r to g_r.  In float, each operation rounded on its own: d = g_r - o_r per axis, L2 = dx*dx; L2 += dy*dy;
 *     L2 += dz*dz, L = sqrtf(L2).  The ray is SKIPPED, and counted in rays_skipped, in three cases: L2 == 0; L > max_length; on some axis its
 *     end cells (T3) differ by more than 2^11 -- or, counted with this case, some end coordinate's P (T3) does not satisfy |P| < 2^31: no
 *     row lives there, a coordinate that is not finite ends here, and T3 stays inside int64.
 * T3  FIXED POINT, S = 10.  Per coordinate v (a float) and c = (double)cell_size: P = (double)v / c (one IEEE division),
 *     F = (int64)floor(P * 1024.0) (the product is exact), and the doubled odd coordinate X = 2F + 1.  The cell of v is F >> 10 = floor(P):
 *     exactly the cell the search grid gives a row for an edge of c.  Cell planes lie at multiples of W = 2^11 in X units.  X is odd, so no
 *     end of a ray lies on a plane.
 * T4  THE WALK, in integers only.  A = X(o_r), B = X(g_r).  Per axis a: d_a = |B_a - A_a|, the sign of B_a - A_a,
 *     left_a = |cell(B_a) - cell(A_a)|, and n_a = the distance in X units from A_a to the first plane in the direction of travel (odd, at
 *     least 1).  The walk starts in the origin's cell, which is traversed.  While some left_a > 0: among the axes with left_a > 0 take the
 *     smallest crossing parameter n_a / d_a, compared by cross-multiplication n_a * d_b < n_b * d_a in int64 (T2 bounds the products below
 *     2^47); EVERY axis tied for the smallest steps at once (cell_a += sign_a, n_a += W, left_a -= 1); the cell reached is traversed.  A cell
 *     the segment touches only at an edge or corner is therefore never traversed.  The walk ends in the endpoint's cell by construction,
 *     after at most 3 * 2^11 steps.  The traversed set is exactly the cells whose open box meets the segment.  Cells outside [-2^20, 2^20)
 *     hold no rows.
 * T5  CANDIDATES AND THE PAIR TEST.  The candidates of ray r are the retained rows j != r (by row index) that lie in a traversed cell.  In
 *     float, each operation rounded on its own, with u = g_r - p_j per axis: rem = ux*dx; rem += uy*dy; rem += uz*dz; rem = rem / L (the
 *     foot's distance before the endpoint, taken endpoint-relative so that the cancellation is small where the cone is narrow);
 *     u2 = ux*ux; u2 += uy*uy; u2 += uz*uz; perp2 = u2 - rem*rem; s = L - rem; w = tan_half_angle * rem.  Ray r SEES THROUGH row j iff all
 *     four hold: s >= start_margin; rem >= end_margin; perp2 <= rho*rho; perp2 <= w*w.  NaNs fail every comparison.
 * T6  COUNTS AND FLAGS.  passes_j is the number of rays that see through row j, a uint32.  Integer addition is associative: any split over
 *     lanes, waves and atomics gives the same counts, and the same bytes on every run.  Row j is TRANSIENT iff passes_j >= min_passes.
 * T7  THE STORE.  A classification stays valid until a scan is added or the store is compacted, by this feature or by O6.
 *     dmsa_dense_cloud_remove_transients compacts points and origins to the non-transient rows, stably, exactly as O6 does.  Afterwards the
 *     grid, the normals, the outlier classification and this classification are all invalid.  The voxel set and dmsa_dense_stats are
 *     untouched.
 *
 * THE HASH of a walk (the stage call): h = 0xCBF29CE484222325; for every traversed cell in walk order, for a = x, y, z:
 * h = (h ^ (uint64)(int64)(cell_a + 2^20)) * 0x100000001B3, modulo 2^64.
 *
 * THE DEFAULTS come from a synthetic toy scene (a ground plane, a wall and a walking box), not from recorded data.
 */
#ifndef DMSA_DENSE_CARVE_H
#define DMSA_DENSE_CARVE_H

#include "dmsa_dense_outliers.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmsa_dense_carve_config {
    float   cell_size;       /* 0.2: metres; edge of the cells the rays are walked through (T3)            */
    float   rho;             /* 0.1: metres; largest distance of a seen-through point from the ray          */
    float   tan_half_angle;  /* 0.052407779: the float nearest tan 3 deg; the cone at the endpoint (T5)     */
    float   end_margin;      /* 0.3: metres; the foot lies at least this far before the endpoint            */
    float   start_margin;    /* 0.5: metres; ... and at least this far behind the origin                    */
    float   max_length;      /* 30:  metres; longer rays are skipped (T2)                                   */
    int32_t min_passes;      /* 2:   rays that must see through a row to call it transient, 1 .. 2^20       */
    int32_t pad;
} dmsa_dense_carve_config;
void dmsa_default_dense_carve_config(dmsa_dense_carve_config* cfg);

typedef struct dmsa_dense_carve_stats {
    int64_t rows, rays_walked, rays_skipped; /* rows = rays_walked + rays_skipped                       */
    int64_t cells_traversed;                 /* summed over the walked rays                             */
    int64_t pair_tests, seen_through;        /* candidates offered (T5) / the sum of passes (T6)        */
    int64_t transient, kept;                 /* rows = transient + kept                                 */
} dmsa_dense_carve_stats;

/* Host only, no context: T2's skip test, then T3 and T4 for the one ray o -> g (max_length is no argument: of T2's cases the first and the
 * third apply here, the second is dmsa_dense_carve_sees_through's and the stage call's).  *n = cells
 * traversed, -1 for a skipped ray; the first min(*n, cap) cells go to cells_xyz (x y z each; may be NULL with cap 0).  A cell_size that is
 * not finite or not > 0, a NULL o, g or n, cap < 0: DMSA_ERR_INVALID. */
int dmsa_dense_carve_walk(float cell_size, const float* o, const float* g, int32_t* cells_xyz, int64_t cap, int64_t* n);
/* Host only: T2's L and T5 for ray o -> g and point p.  1 = sees through, 0 = does not (a ray with L2 == 0 or L > max_length sees
 * through nothing); DMSA_ERR_INVALID (negative) for a config T1 refuses (cell_size is not looked at) or a NULL argument. */
int dmsa_dense_carve_sees_through(const dmsa_dense_carve_config* cfg, const float* o, const float* g, const float* p);
/* The stage call: the device walk for rows [first, first + count): n_cells[i] = cells traversed (-1 = skipped, T2 with cfg->max_length),
 * cell_hash[i] = THE HASH of the sequence (0 for a skipped ray).  Either output may be NULL. */
int dmsa_dense_cloud_carve_walk_rows(dmsa_dense_cloud* dc, const dmsa_dense_carve_config* cfg, int64_t first, int64_t count, int32_t* n_cells, uint64_t* cell_hash);
/* T2-T6 for every retained row.  passes_out (rows uint32) and stats may be NULL; the flags stay in HBM for
 * dmsa_dense_cloud_remove_transients. */
int dmsa_dense_cloud_count_passes(dmsa_dense_cloud* dc, const dmsa_dense_carve_config* cfg, uint32_t* passes_out, dmsa_dense_carve_stats* stats);
/* T7.  Needs a count that is still valid (none yet, a scan added since, or the store compacted since: DMSA_ERR_INVALID).  *kept (optional)
 * = rows left in the store.  The cleaned store is written with dmsa_dense_cloud_save_pcd_retained. */
int dmsa_dense_cloud_remove_transients(dmsa_dense_cloud* dc, int64_t* kept);

#ifdef __cplusplus
}
#endif
#endif /* DMSA_DENSE_CARVE_H */
