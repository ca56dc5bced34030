// dense_align_plane.h — launcher of the kernel behind include/dmsa_dense_align_plane.h (csrc/dense_align_plane.hip): P2's exact sums of the
// pairs that k_nearest_across found in the completeness direction, with the store's normals.  The transform, the grids, the search and D4's
// sums are the kernels of csrc/dense_compare.h, unchanged.
#pragma once
#include "dense_compare.h"

namespace dmsa {

constexpr int kAlignPlaneSums = 64;  // DMSA_ALIGN_PLANE_SUMS, in P2's order

// sums[0..64) += P2's sums over the reference rows i < n with best[i] != kCompareNoMatch and ref_valid[i] != 0: p = ref_pts[i], g =
// store_pts[j] and the normal store_normals[j] (x, y, z; w is not read) with j = the low word of best[i] (a row below store_rows), p and g
// quantised with scale_c.  `sums` is zeroed by the caller.
void launch_align_plane_sums(const unsigned long long* best, const float4* ref_pts, const uint8_t* ref_valid, const float4* store_pts, const float4* store_normals,
                             int64_t store_rows, int64_t n, float scale_c, unsigned long long* sums, hipStream_t s);
}  // namespace dmsa
