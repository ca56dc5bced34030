// dense_align.h — launchers of the kernels behind include/dmsa_dense_align.h and include/dmsa_dense_align_plane.h (csrc/dense_align.hip):
// A2's and P2's exact sums of the pairs that k_nearest_across found in the completeness direction, the latter with the store's normals.  The
// transform, the grids, the search and D4's sums are the kernels of csrc/dense_compare.h, unchanged.
#pragma once
#include "dense_compare.h"

namespace dmsa {

constexpr int kAlignSums = 25;       // DMSA_ALIGN_SUMS: n, Sp[3], Sg[3], then lo, hi of the nine Spg[a][b], a-major
constexpr int kAlignPlaneSums = 64;  // DMSA_ALIGN_PLANE_SUMS, in P2's order

// sums[0..25) += A2's sums over the reference rows i < n with best[i] != kCompareNoMatch and ref_valid[i] != 0: p = ref_pts[i], g =
// store_pts[low word of best[i]] (a row below store_rows), both quantised with scale_c.  `sums` is zeroed by the caller.
void launch_align_pair_sums(const unsigned long long* best, const float4* ref_pts, const uint8_t* ref_valid, const float4* store_pts, int64_t store_rows, int64_t n,
                            float scale_c, unsigned long long* sums, hipStream_t s);
// sums[0..64) += P2's sums over the same rows: p, g and the normal store_normals[j] (x, y, z; w is not read) of g's row j.
void launch_align_plane_sums(const unsigned long long* best, const float4* ref_pts, const uint8_t* ref_valid, const float4* store_pts, const float4* store_normals,
                             int64_t store_rows, int64_t n, float scale_c, unsigned long long* sums, hipStream_t s);
}  // namespace dmsa
