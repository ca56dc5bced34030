// dense_normals.h — launchers of the kernels behind include/dmsa_dense_normals.h (csrc/dense_normals.hip): the exact integer moments of every
// radius neighbourhood over the search grid of csrc/dense_grid.h, the normals and the 28- or 32-byte rows of their file.
#pragma once
#include "dense_grid.h"

namespace dmsa {

// N2-N3 for the retained rows [first, first + count): moments[(row - first) * 10 + 0..9]
void launch_neighbour_moments(const GridView& grid, float r2, float scale, int64_t first, int64_t count, long long* moments, hipStream_t s);
// N4 for rows [first, first + count): normal[first + i] from moments[10 i ..]; *without += rows that got NaNs
void launch_normals_from_moments(const long long* moments, const float4* g, const float4* origin, int64_t first, int64_t count, int32_t min_neighbours,
                                 float4* normal, unsigned long long* without, hipStream_t s);
// row_floats = 7: rows[7 k .. 7 k + 6] = g[first + k].xyz, normal[first + k] (nx, ny, nz, curvature); 8: g[first + k] whole (x y z intensity), then the normal
void launch_pack_normal_rows(const float4* g, const float4* normal, int64_t first, int64_t m, int row_floats, float* rows, hipStream_t s);

}  // namespace dmsa
