/*
 * dmsa_dense_align.h — C ABI of the ALIGNMENT of the reference cloud (include/dmsa_dense_compare.h, D0) to the dense cloud: a rigid fine
 * registration by ICP (iterative closest point, point to point) that produces the 3 x 4 alignment T which dmsa_dense_cloud_set_reference
 * takes.  What CloudCompare's or PCL's fine registration does for a surveyed ground-truth cloud or the map of another run, on the points
 * where they already are.  The start must lie inside ICP's basin: there is no coarse or global registration here, no scale and no
 * trimming by rank.  The point-to-plane residual is a second entry of its own, include/dmsa_dense_align_plane.h (P0-P9).
 *
 * Like D0-D8 the semantics are DECIDED HERE, stated below, and tested against an independent model (tests/dense_align_model.py).  The sums of
 * a rigid fit are integers, the step is one stated sequence of double operations on the host, so the result does not depend on how lanes,
 * waves or atomics interleave: the same inputs give the same bytes on every run.  Same conventions as dmsa_hip.h (contexts, status codes, no
 * CPU fallback).  An object that never aligns allocates and launches what it did before.
 *
 * A0  INPUTS AND PRECONDITIONS.  dmsa_dense_cloud_align_reference takes the caller's reference rows exactly as D0 does (n <= 2^26 host rows
 *     of stride_floats >= 3 floats, here n >= 1) and a start T0, row-major 3 x 4, finite; T0 == NULL is the identity.  D1's preconditions
 *     on cfg.max_distance (retention on, at least one retained row, voxel_size > 0, max_distance finite and in [voxel_size, 64 * voxel_size],
 *     retained rows <= 2^26); 1 <= max_iterations <= DMSA_ALIGN_MAX_ITERATIONS (64); min_pairs >= 3; stop_translation and stop_rotation
 *     finite and >= 0.  Anything else: DMSA_ERR_INVALID with the reason in dmsa_last_error.  The raw rows are uploaded once, live on the
 *     device for the duration of the call and are released with it, as set_reference releases them.
 * A1  AN ITERATION k holds T_k as twelve doubles.  The reference is transformed FROM THE RAW ROWS with T_k by D0's rule (the twelve doubles
 *     cast to float, rule 5's form, also when T_k is the identity), never from the previous iterate's floats; validity is D0's; the reference's
 *     grid is rebuilt.  The pairs of the iteration are D2's in D3's completeness direction: every valid transformed reference row p_i with
 *     its nearest store row g_j within max_distance.  Unmatched and invalid rows take no part.
 * A2  EXACT SUMS.  frexpf(voxel_size) = m * 2^e, scale_c = 2^(10 - e).  Per coordinate P = (int32)rintf(p * scale_c) and G alike: the
 *     product is exact, and rule 6's bound gives |P|, |G| <= 2^30.  Over the pairs: n; Sp[a] = sum P_a; Sg[b] = sum G_b; nine Spg[a][b] =
 *     sum P_a * G_b.  A product is below 2^60 in magnitude and a sum of up to 2^26 of them below 2^86, so each Spg is carried as two int64
 *     words, lo = sum (prod & 0xFFFFFFFF) < 2^58 and hi = sum (prod >> 32) (an arithmetic shift), |hi| < 2^54; its value is hi * 2^32 + lo.
 *     The linear sums are below 2^56 and fit one word.  25 int64 words, in this order: n, Sp[0..2], Sg[0..2], then for a = 0..2, b = 0..2 the
 *     pair lo, hi of Spg[a][b] (DMSA_ALIGN_SUMS).  Integer addition is associative: any split gives the same 25 words.  D4's sums of the
 *     same pairs (matched, unmatched, s1, s2 at D4's own scale) come along unchanged.
 * A3  THE STEP, on the host (dmsa_dense_align_solve), in double, without contraction, each operation rounded on its own.
 *     M[a][b] = n * Spg[a][b] - Sp[a] * Sg[b], EXACTLY in 128-bit integers (below 2^113), each converted to double once, to nearest even.
 *     mx = the largest |M[a][b]|; S = M / mx entry by entry (mx == 0: the rotation is the identity, q = (1, 0, 0, 0)).  Horn's symmetric
 *     matrix, rows and columns (w, x, y, z):
 *         N00 = (S00 + S11) + S22   N01 = S12 - S21           N02 = S20 - S02           N03 = S01 - S10
 *                                   N11 = (S00 - S11) - S22   N12 = S01 + S10           N13 = S20 + S02
 *                                                             N22 = (S11 - S00) - S22   N23 = S12 + S21
 *                                                                                       N33 = (S22 - S00) - S11
 *     Cyclic Jacobi on A = N with V = I, at most 16 sweeps; a sweep starts only while off = ((((A01^2 + A02^2) + A03^2) + A12^2) + A13^2) +
 *     A23^2 is not exactly 0; within a sweep (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a pair with A[p][q] == 0 is skipped; otherwise
 *         theta = (A[q][q] - A[p][p]) / (2 * A[p][q]);  r = fabs(theta) + sqrt(theta * theta + 1);  t = theta < 0 ? -1 / r : 1 / r;
 *         c = 1 / sqrt(t * t + 1);  s = t * c;
 *         A[p][p] -= t * A[p][q];  A[q][q] += t * A[p][q] (the old A[p][q]);  A[p][q] = A[q][p] = 0;
 *         for the two r other than p and q:  A[r][p] = A[p][r] = c * a_rp - s * a_rq,  A[r][q] = A[q][r] = s * a_rp + c * a_rq (old values);
 *         for r = 0..3:                      V[r][p] = c * v_rp - s * v_rq,            V[r][q] = s * v_rp + c * v_rq.
 *     Only + - * /, sqrt and fabs.  The column of V at the largest A[i][i] is taken (a tie: the lowest column), divided by its norm
 *     sqrt(((v0^2 + v1^2) + v2^2) + v3^2), and negated if w < 0, or if w == 0 and the first non-zero of x, y, z is negative.
 *     With xx = x*x, yy, zz, xy = x*y, xz, yz, wx = w*x, wy, wz:
 *         R00 = 1 - 2 * (yy + zz)   R01 = 2 * (xy - wz)       R02 = 2 * (xz + wy)
 *         R10 = 2 * (xy + wz)       R11 = 1 - 2 * (xx + zz)   R12 = 2 * (yz - wx)
 *         R20 = 2 * (xz - wy)       R21 = 2 * (yz + wx)       R22 = 1 - 2 * (xx + yy)
 *     pm[a] = (double)Sp[a] / (double)n, gm alike;  dt[a] = (gm[a] - ((R[a][0] * pm[0] + R[a][1] * pm[1]) + R[a][2] * pm[2])) / scale_c.
 *     Because the sums carry no scale_c of their own, dmsa_dense_align_solve returns dt in QUANTISED UNITS when called alone: it takes
 *     scale_c as an argument (1.0 leaves the units as they are).
 * A4  MEASURES OF A STEP, free of the lever arm to the origin.  shift = sqrt((s0^2 + s1^2) + s2^2) with s[a] = (gm[a] - pm[a]) / scale_c:
 *     how far the pairs' centroid moves, because the optimal step maps centroid to centroid.  rotation = 2 * sqrt((x^2 + y^2) + z^2): the
 *     angle for small steps, no trigonometry.
 * A5  COMPOSITION.  T_{k+1} = D o T_k in double: entry (a, c) = (D[a][0] * T[0][c] + D[a][1] * T[1][c]) + D[a][2] * T[2][c], plus D[a][3]
 *     for c = 3 (rule 5's bracket order).  There is no re-orthonormalisation: 64 products of rotations that are orthonormal to a few ulp
 *     drift by some 1e-14, far below the float cast of D0.
 * A6  STOPPING, tested in this order.  DMSA_ALIGN_STOP_TOO_FEW_PAIRS: n < min_pairs; the iteration gives no step, T_k is the result (its
 *     shift_m and rotation_rad are reported as 0).  DMSA_ALIGN_STOP_CONVERGED: shift <= stop_translation and rotation <= stop_rotation;
 *     the step that met the test is still applied, the result is T_{k+1}.  DMSA_ALIGN_STOP_MAX_ITERATIONS: max_iterations steps have been
 *     applied.  There is no "stalled" rule: pairs that enter the reach as the clouds close in raise the mean distance legitimately, and a
 *     monotonicity test would stop a partial overlap early.
 * A7  THE STATE AFTERWARDS is exactly what dmsa_dense_cloud_set_reference(dc, xyz, n, stride_floats, T_result) would have left, byte for
 *     byte: the transformed rows, validity, ref_invalid, results against the old reference stale.  A refused or failed call leaves no
 *     reference, as D0's failure path does (a call refused for a null object or a null output touches nothing).
 * A8  THE REPORT: iterations (the entries of `history`: the iterations whose pairs were searched), stop, scale_c, per iteration matched,
 *     unmatched, s2 (D4's), rms_m (D5's expression), shift_m, rotation_rad; the last iteration's 25 sums; T, the twelve doubles of the
 *     result (also written to T_out).
 *
 * A LIMIT, stated and not lifted here: D0 applies T in float.  A map tens of kilometres from its origin cannot be aligned finer than the float
 * rounding of T times the coordinates allows: a CPU prototype of these rules on a room offset by 90 km at 0.1 m voxels jittered at an rms of
 * 0.019-0.024 m against 0.0173 m converged at the origin, and ran to DMSA_ALIGN_STOP_MAX_ITERATIONS.  That belongs to D0.
 */
#ifndef DMSA_DENSE_ALIGN_H
#define DMSA_DENSE_ALIGN_H

#include "dmsa_dense_compare.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DMSA_ALIGN_MAX_ITERATIONS 64
#define DMSA_ALIGN_SUMS 25
#define DMSA_ALIGN_STOP_CONVERGED 0
#define DMSA_ALIGN_STOP_MAX_ITERATIONS 1
#define DMSA_ALIGN_STOP_TOO_FEW_PAIRS 2

/* The defaults are placeholders from a synthetic room (an 8 x 6 x 3 m box at 0.1 m voxels with 1 cm noise), not from recorded data. */
typedef struct dmsa_dense_align_config {
    float   max_distance;      /* 1.0: metres; the reach of the pairs (A1, D2)                       */
    int32_t max_iterations;    /* 30                                                                 */
    int32_t min_pairs;         /* 3                                                                  */
    int32_t pad;
    double  stop_translation;  /* 1e-4: metres (A4's shift)                                          */
    double  stop_rotation;     /* 1e-5: radians (A4's rotation)                                      */
} dmsa_dense_align_config;
void dmsa_default_dense_align_config(dmsa_dense_align_config* cfg);

typedef struct dmsa_dense_align_iteration {
    int64_t matched, unmatched, s2;
    double  rms_m, shift_m, rotation_rad;
} dmsa_dense_align_iteration;

typedef struct dmsa_dense_align_report {
    int32_t iterations, stop;
    double  scale_c;
    dmsa_dense_align_iteration history[DMSA_ALIGN_MAX_ITERATIONS];
    int64_t sums[DMSA_ALIGN_SUMS];
    double  T[12];
} dmsa_dense_align_report;

/* A0-A8.  T_out (12 doubles) and report may be NULL. */
int dmsa_dense_cloud_align_reference(dmsa_dense_cloud* dc, const float* xyz, int64_t n, int32_t stride_floats, const double* T0, const dmsa_dense_align_config* cfg,
                                     double* T_out, dmsa_dense_align_report* report);
/* The stage call: A2's sums of the reference AS IT STANDS (dmsa_dense_cloud_set_reference) against the store as it stands, and D4's block of
 * the same pairs (d4 may be NULL; its histogram and `within` are at tolerance = max_distance).  Of cfg only max_distance is read.  D1's
 * preconditions. */
int dmsa_dense_cloud_align_sums(dmsa_dense_cloud* dc, const dmsa_dense_align_config* cfg, int64_t sums[DMSA_ALIGN_SUMS], dmsa_dense_compare_direction* d4);
/* A3-A4, host only, no context.  dT: the step, row-major 3 x 4; shift_m and rotation_rad may be NULL.  scale_c: A2's, finite and > 0.  Sums
 * outside A2's ranges (n < 1 or > 2^26, |Sp|, |Sg| > n * 2^30, lo outside [0, n * 2^32), |hi| > n * 2^28): DMSA_ERR_INVALID. */
int dmsa_dense_align_solve(const int64_t sums[DMSA_ALIGN_SUMS], double scale_c, double dT[12], double* shift_m, double* rotation_rad);
/* A5, host only: out = D o T (out may be D or T). */
int dmsa_dense_align_compose(const double D[12], const double T[12], double out[12]);
/* A2: scale_c of a voxel_size (0 for a voxel_size that is not finite and positive). */
double dmsa_dense_align_scale(float voxel_size);

#ifdef __cplusplus
}
#endif
#endif /* DMSA_DENSE_ALIGN_H */
