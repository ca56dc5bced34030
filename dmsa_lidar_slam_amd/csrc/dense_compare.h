// dense_compare.h — launchers of the kernels behind include/dmsa_dense_compare.h (csrc/dense_compare.hip): the reference cloud's transform and
// validity, its cell keys, the nearest row of one point set for the queries of another over two search grids of csrc/dense_grid.h cut with
// the same edge, and the exact sums, the histogram and the flags.  The compaction and the rows of the file are the kernels of
// csrc/dense_cloud.h.
#pragma once
#include "dense_grid.h"

namespace dmsa {

// the words of one direction's sums block in HBM, zeroed before the launch that adds to it; the 64 bins follow CM_BINS
enum CompareSum { CM_MATCHED = 0, CM_S1, CM_S2, CM_UNMATCHED, CM_WITHIN, CM_KEPT, CM_BINS, CM_COUNT = CM_BINS + 64 };
// D2's key of a query without a candidate (every real key is below it: the bits of a finite d2 are below 0x7F800000)
constexpr unsigned long long kCompareNoMatch = ~0ull;

struct RefTransform {
    float c[12];  // row-major 3 x 4
};

// D0: pts[i] = (T applied to row i of `raw` in rule 5's form, or the row itself; w = 0), valid[i] = the row is finite and inside rule 6's
// grid at voxel_size; *invalid += the rows that are not
void launch_reference_transform(const float* raw, int64_t n, int32_t stride_floats, bool transform, RefTransform T, float voxel_size, float4* pts, uint8_t* valid,
                                unsigned long long* invalid, hipStream_t s);
// launch_grid_cell_keys for the reference: an invalid row gets the key ~0 and sorts behind every valid row (a sort over all 64 bits)
void launch_reference_cell_keys(const float4* pts, const uint8_t* valid, int64_t n, double cell, unsigned long long* key, uint32_t* idx, hipStream_t s);
// D2, the hot kernel: for the queries of grid `q` whose original row lies in [first, first + count), best[row - first] = the smallest
// (bits(d2) << 32) | original row of `in` over the rows of `in` with d2 <= r2.  `best` is set to kCompareNoMatch by the caller: rows that are
// in neither grid keep it.
void launch_nearest_across(const GridView& q, const GridView& in, float r2, int64_t first, int64_t count, unsigned long long* best, hipStream_t s);
// D2's dist and index and D4 from the keys of n queries: dist[i] = sqrtf(d2) or NaN, index[i] = the row or -1, sums += this launch's share.
// valid (may be null: every query counts) leaves the queries with valid[i] == 0 out of every sum.  tol_bits = the bits of the float
// tolerance * tolerance.
void launch_compare_quantise_sum(const unsigned long long* best, const uint8_t* valid, int64_t n, float scale, uint32_t tol_bits, float* dist, int32_t* index,
                                 unsigned long long* sums, hipStream_t s);
// D6: keep[i] = flag8[i] = (matched and d2 <= tolerance^2) == near; keep[n] = 0; sums[CM_KEPT] += the rows kept
void launch_compare_flags(const unsigned long long* best, int64_t n, uint32_t tol_bits, bool near, int32_t* keep, uint8_t* flag8, unsigned long long* sums,
                          hipStream_t s);
}  // namespace dmsa
