// dense_carve.h — launchers of the kernels behind include/dmsa_dense_carve.h (csrc/dense_carve.hip): every retained ray walked through the
// search grid of csrc/dense_grid.h (T2-T4), the rows of the traversed cells put to the pair test (T5), the counts (T6) and the flags.
// The compaction is the kernels of csrc/dense_cloud.h.
#pragma once
#include "dense_grid.h"

namespace dmsa {

// the scalars of dmsa_dense_carve_config the kernels read
struct CarveParams {
    double cell;  // (double)cell_size: the edge the grid was built with
    float rho, tan_half_angle, end_margin, start_margin, max_length;
};
// the words of the sums block in HBM, zeroed before k_carve_passes
enum CarveSum { CS_SKIPPED = 0, CS_CELLS, CS_PAIRS, CS_SEEN, CS_COUNT };

// T2-T4 for the store's rows [first, first + count): n_cells[i] = cells traversed or -1, hash[i] = the header's hash of the walk
void launch_carve_walk_rows(const float4* g, const float4* origin, int64_t first, int64_t count, CarveParams p, int32_t* n_cells, unsigned long long* hash, hipStream_t s);
// T2-T6 for all n rows: passes[j] += rays that see through row j (zeroed by the caller), sums[CS_*] += this launch's share
void launch_carve_passes(const GridView& grid, const float4* origin, CarveParams p, uint32_t* passes, unsigned long long* sums, hipStream_t s);
// keep[i] = passes[i] < min_passes; keep[n] = 0 (the scan over n + 1 flags ends in the number of rows kept)
void launch_carve_flags(const uint32_t* passes, int64_t n, uint32_t min_passes, int32_t* keep, hipStream_t s);

}  // namespace dmsa
