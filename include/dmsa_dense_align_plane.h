/*
 * dmsa_dense_align_plane.h — C ABI of the POINT-TO-PLANE alignment of the reference cloud to the dense cloud: the second entry beside
 * include/dmsa_dense_align.h (point to point, A0-A8).  The residual of a pair is its distance along the store row's normal
 * (include/dmsa_dense_normals.h, N4), which lets the reference slide along a surface and so takes a fraction of the iterations.  Nothing of
 * A0-A8 changes: dmsa_dense_cloud_align_reference, its structs, its 25 sums and its kernel are what they were.
 *
 * Like A0-A8 the semantics are DECIDED HERE, stated below, and tested against an independent model (tests/dense_align_plane_model.py).  The
 * sums of a point-to-plane step are integers: products of THREE quantised values, carried in 32-bit limbs whose sums fit int64 words.  The
 * step is one stated sequence of double operations on the host.  The same inputs give the same bytes on every run, whatever lanes, waves and
 * atomics do.  An object that never calls this allocates and launches what it did before.
 *
 * P0  INPUTS AND PRECONDITIONS.  Everything A0 asks, with min_pairs >= 6 (six unknowns).  The store's normals must be valid: a completed
 *     dmsa_dense_cloud_compute_normals since the store last changed (a scan added, rows removed).  Anything else: DMSA_ERR_INVALID with the
 *     reason in dmsa_last_error.  A refused or failed call leaves no reference, as A7 says.
 * P1  THE PAIRS of an iteration are A1's, unchanged: T_k is twelve doubles, the reference is transformed from the raw rows by D0, its grid is
 *     rebuilt, the pairs are D3's completeness direction within max_distance.  A matched pair is USED iff the store row has a normal: its three
 *     floats n_a are finite, and with N_a = rint(n_a * 2^14) the integer Nx^2 + Ny^2 + Nz^2 lies in [2^27, 2^29] (a length in [0.707, 1.414]:
 *     N4 gives unit normals, a row below min_neighbours holds NaNs).  A component with |n_a * 2^14| > 2^15 fails that test by itself and is never
 *     converted.  A matched pair without a normal is counted in no_normal and takes no other part.  D4's block of ALL matched pairs comes
 *     along unchanged: matched = used + no_normal.
 * P2  EXACT SUMS.  P and G are quantised exactly as A2 does: scale_c = 2^(10 - e), P = (int32)rintf(p * scale_c), |P|, |G| <= 2^30.  Per used
 *     pair, all in integers:  c = P x N (c_x = Py*Nz - Pz*Ny, c_y = Pz*Nx - Px*Nz, c_z = Px*Ny - Py*Nx)  and  e = (G - P) . N.
 *     BOUNDS.  |N| <= 2^14.5 (its square is at most 2^29), so |N_a| <= 2^14.5 and |N_a N_b| <= 2^29.  Two coordinates of P have a length of
 *     at most 2^30.5 and so |c_a| <= 2^30.5 * 2^14.5 = 2^45.  The pair lies within max_distance <= 64 * voxel_size < 2^16 / scale_c, each
 *     quantisation moves a coordinate by at most 1/2, the float test of D2 admits a few parts in 2^24: |G - P| < 2^16 + 2 as a vector, and
 *     |e| <= |G - P| |N| < 2^30.6 < 2^31.  Hence, per pair, |c_a N_b| < 2^60, |c_a c_b| <= 2^90 < 2^91, |N_a e| < 2^46, |c_a e| < 2^76 < 2^77,
 *     e^2 < 2^62.
 *     LIMBS (A2's lo / hi form, generalised).  A product x is carried in W words: limb k < W - 1 is (x >> 32k) & 0xFFFFFFFF, the top limb is
 *     x >> 32(W - 1), an arithmetic shift; the value is sum limb_k * 2^(32k).  A lower limb is below 2^32 and the top limbs above are below
 *     2^28, 2^27, 2^14, 2^13 and 2^30 in magnitude: every limb sum over at most 2^26 pairs is below 2^58 and fits an int64.
 *     64 int64 words (DMSA_ALIGN_PLANE_SUMS), in this order:
 *         [0]       n, the used pairs                       [1]       no_normal
 *         [2..4]    Sp[a] = sum P_a                         [5..10]   sum N_a N_b for xx xy xz yy yz zz, one word each
 *         [11..28]  sum c_a N_b, nine entries a-major, 2 limbs each (lo, hi)
 *         [29..46]  sum c_a c_b for xx xy xz yy yz zz, 3 limbs each
 *         [47..52]  sum N_a e, 2 limbs each                 [53..61]  sum c_a e, 3 limbs each          [62..63]  sum e^2, 2 limbs
 *     Integer addition is associative: any split gives the same 64 words.  Flipping a normal's sign flips c and e together, and every word
 *     holds an even number of them: the sums do not depend on how the normals are oriented.
 * P3  RE-CENTRING, exact, on the host.  Sums about the origin cannot be solved in double for a map far from it; they are integers, so the
 *     pivot is moved exactly.  C_a = floor((2 * Sp_a + n) / (2 n)), the rounded mean of the P.  c' = (P - C) x N = c - K N with K = [C]x
 *     (rows (0, -Cz, Cy), (Cz, 0, -Cx), (-Cy, Cx, 0)).  In 128-bit integers, from the groups above:
 *         (c'N)[a][b] = (cN)[a][b] - sum_k K[a][k] (NN)[k][b]
 *         (c'c')[a][b] = (cc)[a][b] - sum_k K[a][k] (cN)[b][k] - sum_k (c'N)[a][k] K[b][k]
 *         (c'e)[a] = (ce)[a] - sum_k K[a][k] (Ne)[k]
 *     The sums are below 2^26 * 2^60 = 2^86 (cN), 2^55 (NN), 2^117 (cc), 2^72 (Ne), 2^103 (ce); |K| <= 2^30 with two entries per row: every
 *     intermediate is below 2^120.  The system is the symmetric 6 x 6 integer matrix A = [[c'c', c'N], [(c'N)^T, NN]] (unknowns omega, then
 *     t) and b = [c'e; Ne]; each entry is converted to double once, to nearest even.
 * P4  THE STEP, on the host (dmsa_dense_align_plane_solve), in double, without contraction, each operation rounded on its own; only + - * /
 *     and sqrt.  Scaling: s_i = 1 / sqrt(A_ii); an A_ii that is not > 0 is DEGENERATE (min_pivot 0).  For i >= j: M_ij = (A_ij * s_i) * s_j;
 *     r_i = b_i * s_i.  LDL^T without pivoting, for j = 0..5:
 *         v = M_jj;  for k = 0..j-1:  v = v - (L_jk * D_k) * L_jk;   D_j = v;   D_j not > 2^-40: DEGENERATE (min_pivot D_j);
 *         for i = j+1..5:  u = M_ij;  for k = 0..j-1:  u = u - (L_ik * D_k) * L_jk;   L_ij = u / D_j.
 *     The scaled matrix has a unit diagonal, so D_j is the share of column j that the columns before it do not explain.  2^-40 sits three
 *     orders above the roundoff of the factorisation and far below anything data gives: it catches rank deficiency ONLY and is no
 *     observability judgement.  min_pivot = the smallest D_j.  Then for i = 0..5: y_i = r_i, for k = 0..i-1: y_i = y_i - L_ik * y_k;
 *     z_i = y_i / D_i; for i = 5..0: x_i = z_i, for k = i+1..5: x_i = x_i - L_ki * x_k; finally x_i = x_i * s_i: omega = x_0..2
 *     (dimensionless), t = x_3..5 in quantised units.
 *     The rotation has no trigonometry: h = omega * 0.5, nr = sqrt(((1 + hx*hx) + hy*hy) + hz*hz), q = (1 / nr, hx / nr, hy / nr, hz / nr), R
 *     from q by A3's formula.  Its angle is 2 atan(|omega| / 2), which differs from |omega| in third order: the fixed point of an iterated
 *     step does not move.  dt_a = ((C_a + t_a) - ((R_a0 * C_0 + R_a1 * C_1) + R_a2 * C_2)) / scale_c: the rotation turns about the pivot.
 *     dmsa_dense_align_plane_solve takes scale_c as an argument (1.0 leaves quantised units).
 * P5  MEASURES OF A STEP.  shift = sqrt((t0^2 + t1^2) + t2^2) / scale_c: how far the pivot moves.  rotation = 2 * sqrt((x^2 + y^2) + z^2) of q.
 * P6  COMPOSITION is A5 (dmsa_dense_align_compose), unchanged.
 * P7  STOPPING, tested in this order.  DMSA_ALIGN_STOP_TOO_FEW_PAIRS: used pairs < min_pairs; no step, T_k is the result.
 *     DMSA_ALIGN_STOP_DEGENERATE (3): P4 said so; no step is applied, T_k is the result, min_pivot is reported, shift and rotation are 0.
 *     DMSA_ALIGN_STOP_CONVERGED: shift <= stop_translation and rotation <= stop_rotation; the step that met the test is still applied.
 *     DMSA_ALIGN_STOP_MAX_ITERATIONS.
 *     WHAT THIS DOES NOT DETECT.  Noisy normals on a single plane give a system that LOOKS well conditioned (a CPU prototype's smallest pivot
 *     there was 0.98) although the slide along the plane and the turn about its normal are not observable.  This stage does not detect that.
 *     min_pivot is reported per iteration; the judgement is the caller's.
 *     D0's float limit for maps far from their origin stays, as include/dmsa_dense_align.h states it; that limit belongs to D0.  A prototype of
 *     these rules at an offset of 9 km ran to DMSA_ALIGN_STOP_MAX_ITERATIONS with steps jittering at 2e-4 to 7e-4 m.
 * P8  THE STATE AFTERWARDS is A7's: byte for byte what dmsa_dense_cloud_set_reference(dc, xyz, n, stride_floats, T_result) leaves.  The
 *     normals, the store and the other stages are untouched.
 * P9  THE REPORT: iterations, stop, scale_c; per iteration matched, unmatched, s2 (D4's), used, no_normal, rms_m (D5's),
 *     plane_rms_m = sqrt((double)sum e^2 / (double)used) / (scale_c * 2^14) (0 without a used pair), shift_m, rotation_rad, min_pivot (0 where
 *     no solve ran); the last iteration's 64 words; T.
 */
#ifndef DMSA_DENSE_ALIGN_PLANE_H
#define DMSA_DENSE_ALIGN_PLANE_H

#include "dmsa_dense_align.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DMSA_ALIGN_PLANE_SUMS 64
#define DMSA_ALIGN_STOP_DEGENERATE 3
/* what dmsa_dense_align_plane_solve returns for a system P4 calls degenerate: no error, and no step (dT is the identity) */
#define DMSA_ALIGN_PLANE_DEGENERATE 1

/* The defaults are placeholders from a synthetic room (an 8 x 6 x 3 m box at 0.1 m voxels with 1 cm noise), not from recorded data. */
typedef struct dmsa_dense_align_plane_config {
    float   max_distance;      /* 1.0: metres; the reach of the pairs (P1, D2)                       */
    int32_t max_iterations;    /* 30                                                                 */
    int32_t min_pairs;         /* 6                                                                  */
    int32_t pad;
    double  stop_translation;  /* 1e-4: metres (P5's shift)                                          */
    double  stop_rotation;     /* 1e-5: radians (P5's rotation)                                      */
} dmsa_dense_align_plane_config;
void dmsa_default_dense_align_plane_config(dmsa_dense_align_plane_config* cfg);

typedef struct dmsa_dense_align_plane_iteration {
    int64_t matched, unmatched, s2, used, no_normal;
    double  rms_m, plane_rms_m, shift_m, rotation_rad, min_pivot;
} dmsa_dense_align_plane_iteration;

typedef struct dmsa_dense_align_plane_report {
    int32_t iterations, stop;
    double  scale_c;
    dmsa_dense_align_plane_iteration history[DMSA_ALIGN_MAX_ITERATIONS];
    int64_t sums[DMSA_ALIGN_PLANE_SUMS];
    double  T[12];
} dmsa_dense_align_plane_report;

/* P0-P9.  T_out (12 doubles) and report may be NULL. */
int dmsa_dense_cloud_align_reference_plane(dmsa_dense_cloud* dc, const float* xyz, int64_t n, int32_t stride_floats, const double* T0,
                                           const dmsa_dense_align_plane_config* cfg, double* T_out, dmsa_dense_align_plane_report* report);
/* The stage call: P2's sums of the reference AS IT STANDS against the store and its normals as they stand, and D4's block of all matched
 * pairs (d4 may be NULL; its histogram and `within` are at tolerance = max_distance).  Of cfg only max_distance is read.  D1's preconditions
 * and P0's of the normals. */
int dmsa_dense_cloud_align_plane_sums(dmsa_dense_cloud* dc, const dmsa_dense_align_plane_config* cfg, int64_t sums[DMSA_ALIGN_PLANE_SUMS], dmsa_dense_compare_direction* d4);
/* P3-P5, host only, no context.  dT: the step, row-major 3 x 4; shift_m, rotation_rad and min_pivot may be NULL.  scale_c: finite and > 0.
 * Returns DMSA_OK, or DMSA_ALIGN_PLANE_DEGENERATE (dT the identity, shift and rotation 0, min_pivot the pivot that failed), or
 * DMSA_ERR_INVALID for words outside P2's ranges: n < 1, no_normal < 0 or n + no_normal > 2^26, |Sp| > n * 2^30, |NN| > n * 2^29 or a negative
 * diagonal one, a lower limb outside [0, n * 2^32), a top limb beyond n times P2's bound for it (2^28, 2^27, 2^14, 2^13, 2^30), or a
 * negative top limb of sum e^2. */
int dmsa_dense_align_plane_solve(const int64_t sums[DMSA_ALIGN_PLANE_SUMS], double scale_c, double dT[12], double* shift_m, double* rotation_rad, double* min_pivot);

#ifdef __cplusplus
}
#endif
#endif /* DMSA_DENSE_ALIGN_PLANE_H */
