// dense_surface.hip — the kernels of include/dmsa_dense_surface.h: the truncated signed distance field of the dense cloud from its measured
// rays, and its zero set by marching tetrahedra.
//
//   k_surface_clear        every slot of the table empty, sum and n 0
//   k_surface_integrate    S2-S5, the hot kernel: one ray per lane, its segment walked with csrc/dense_carve_walk.h into the table
//   k_surface_flags        a flag per slot that holds a key (scanned by the library's exclusive scan)
//   k_surface_compact      keys and slot numbers of the held slots, side by side (sorted by the library's 64-bit sort: S6)
//   k_surface_list         sum and n per listed cell, the cell's listing index back into its slot, the cells with n >= min_weight
//   k_surface_rows         S7: the 20-byte rows of a chunk of the voxel file
//   k_mesh_mark            S8: one anchor per lane: the triangles of its six tetrahedra counted, a flag per vertex they refer to
//   k_mesh_count           the flagged vertices per lower node (both counts scanned by the library's exclusive scan)
//   k_mesh_emit            S8: the vertices of a node and the triangles of an anchor, welded and oriented
//   k_mesh_face_rows       S9: the 13-byte face rows of a chunk of the mesh file
//
// k_surface_integrate takes its rays in the grid's SORTED row order, as k_occupancy_walk does and for the reason stated at the top of
// dense_carve.hip.  The segment of S3 is at most two truncations long, so the walk state stays in registers and the loop is short.  Per
// traversed cell a lane finds or inserts the key (a 64-bit atomicCAS on the key, linear probing, an all-ones key is empty), then adds 1 to n
// with a 32-bit and q to sum with a 64-bit vector atomicAdd.  Equal cells of a wave are NOT merged before the atomics: no measurement was made
// that would favour the merge.  Every loop has a bound: the walk kCarveMaxSteps, the probe the slot count, the tetrahedra six.  Nothing waits
// for another lane.  A table with more keys than `limit`, or a probe that runs out, sets rec[SW_OVERFLOW]; the wave stops, and the host walks
// again into a larger table.  Integer sums throughout: the result does not depend on lane, wave or atomic order.
//
// The mesh kernels run on the finished listing: they only read it, apart from the flags of k_mesh_mark, a plain byte store of the value 1
// from every writer.  A corner is found through the table (key -> slot -> listing index).  k_mesh_mark and k_mesh_emit decide the triangles
// of a tetrahedron with the one function of dense_surface_rule.h, so they cannot disagree; the scans between them give every vertex and
// every triangle its place, and k_mesh_emit checks each place against the room it was given.  No LDS.  Built with -ffp-contract=off.
#include "dense_surface.h"

#include "dense_grid_walk.h"

namespace dmsa {
namespace {

constexpr int kAgentRelaxed = __ATOMIC_RELAXED;

__global__ __launch_bounds__(kBlock) void k_surface_clear(SurfaceSlot* __restrict__ table, const unsigned long long slots) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < slots) table[i] = SurfaceSlot{kCellEmptyKey, 0ull, 0u, 0u};
}

// the slot that holds `key`, entered if no slot did (*inserted); -1 when every slot held another key
__device__ __forceinline__ int64_t d_surface_find_or_insert(SurfaceSlot* table, const uint32_t mask, const unsigned long long key, bool* inserted) {
    uint32_t slot = (uint32_t)mix64(key) & mask;
#pragma unroll 1
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        unsigned long long prev = __hip_atomic_load(&table[slot].key, kAgentRelaxed, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == kCellEmptyKey) {
            prev = atomicCAS(&table[slot].key, kCellEmptyKey, key);
            if (prev == kCellEmptyKey) {
                *inserted = true;
                return (int64_t)slot;
            }
        }
        if (prev == key) return (int64_t)slot;
        slot = (slot + 1) & mask;
    }
    return -1;
}

__global__ __launch_bounds__(kBlock) void k_surface_integrate(const float4* __restrict__ pts, const uint32_t* __restrict__ idx, const float4* __restrict__ origin,
                                                              const int64_t n, const SurfaceParams p, SurfaceSlot* table, const uint32_t mask,
                                                              const unsigned long long limit, unsigned long long* rec) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t self = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // this lane's sorted row: its ray
    // a wave that starts after the table overflowed has nothing to add: the host walks again
    if (__ballot(__hip_atomic_load(rec + SW_OVERFLOW, kAgentRelaxed, __HIP_MEMORY_SCOPE_AGENT) != 0ull) != 0ull) return;
    unsigned long long skipped = 0ull, cells = 0ull, outside = 0ull;
    CarveWalk w{};
    CarveRay ray{};
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    bool active = false;
    if (self < n) {
        const float4 g = pts[self], o = origin[idx[self]];
        gx = g.x, gy = g.y, gz = g.z;
        ray = carve_ray(o.x, o.y, o.z, g.x, g.y, g.z);
        if (carve_ray_skipped(ray, p.max_length)) {
            skipped = 1ull;
        } else {
            const SurfaceSegment seg = surface_segment(ray, o.x, o.y, o.z, g.x, g.y, g.z, p.truncation);
            if (carve_walk_begin(p.cell, seg.ax, seg.ay, seg.az, seg.bx, seg.by, seg.bz, &w)) active = true;
            else skipped = 1ull;
        }
    }
#pragma unroll 1
    for (int32_t step = 0; step <= kCarveMaxSteps; ++step) {  // (T4: every lane's walk ends before the bound does)
        if (__ballot(active) == 0ull) break;
        const bool inside = active && carve_cell_holds_rows(w);
        bool inserted = false, gave_up = false;
        if (inside) {
            const unsigned long long key = d_cell_key(w.cx + kCellBias, w.cy + kCellBias, w.cz + kCellBias);
            const int64_t slot = d_surface_find_or_insert(table, mask, key, &inserted);
            if (slot < 0) {
                gave_up = true;
            } else {
                const int32_t q = surface_sample(ray, gx, gy, gz, w.cx, w.cy, w.cz, p.cell, p.truncation);
                atomicAdd(&table[slot].n, 1u);
                atomicAdd(&table[slot].sum, (unsigned long long)(long long)q);
            }
        }
        // the keys in the table, counted once per wave and step; past `limit` the table is too full to go on
        const unsigned long long entered = __ballot(inserted);
        if (entered != 0ull && lane == __ffsll((long long)entered) - 1) {
            const unsigned long long now = (unsigned long long)__popcll(entered);
            if (atomicAdd(rec + SW_OCCUPIED, now) + now > limit) gave_up = true;
        }
        if (__ballot(gave_up) != 0ull) {
            if (gave_up) atomicMax(rec + SW_OVERFLOW, 1ull);
            break;  // the whole wave: this walk's sums are discarded
        }
        if (active) {
            ++cells;
            if (!inside) ++outside;
            if (!carve_walk_step(&w)) active = false;
        }
    }
    skipped = wave_sum(skipped), cells = wave_sum(cells), outside = wave_sum(outside);
    if (lane == 0) {
        if (skipped != 0ull) atomicAdd(rec + SW_SKIPPED, skipped);
        if (cells != 0ull) atomicAdd(rec + SW_CELLS, cells);
        if (outside != 0ull) atomicAdd(rec + SW_OUT_OF_RANGE, outside);
    }
}

__global__ __launch_bounds__(kBlock) void k_surface_flags(const SurfaceSlot* __restrict__ table, const unsigned long long slots, int32_t* __restrict__ flag) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i > slots) return;
    flag[i] = i < slots && table[i].key != kCellEmptyKey ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void k_surface_compact(const SurfaceSlot* __restrict__ table, const unsigned long long slots, const int32_t* __restrict__ flag,
                                                            const int32_t* __restrict__ scan, const int64_t m, unsigned long long* __restrict__ key,
                                                            uint32_t* __restrict__ slot_of) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= slots || flag[i] == 0) return;
    const int64_t at = (int64_t)scan[i];
    if (at < 0 || at >= m) return;  // (never: the walk counted the keys it entered)
    key[at] = table[i].key, slot_of[at] = (uint32_t)i;
}

// *sum += `mine` over the wave, one atomic per wave
__device__ __forceinline__ void d_add_wave(unsigned long long mine, unsigned long long* sum) {
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine != 0ull) atomicAdd(sum, mine);
}

__global__ __launch_bounds__(kBlock) void k_surface_list(SurfaceSlot* __restrict__ table, const uint32_t* __restrict__ slot_sorted, const int64_t m,
                                                         const uint32_t min_weight, long long* __restrict__ sum, uint32_t* __restrict__ n,
                                                         unsigned long long* __restrict__ rec) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long valid = 0ull;
    if (j < m) {
        SurfaceSlot* e = table + slot_sorted[j];
        const uint32_t weight = e->n;
        sum[j] = (long long)e->sum, n[j] = weight, e->index = (uint32_t)j;
        valid = weight >= min_weight ? 1ull : 0ull;
    }
    d_add_wave(valid, rec + SW_VALID);
}

__device__ __forceinline__ int d_key_x(const unsigned long long key) { return (int)(key >> 42) & kCellMax; }
__device__ __forceinline__ int d_key_y(const unsigned long long key) { return (int)(key >> 21) & kCellMax; }
__device__ __forceinline__ int d_key_z(const unsigned long long key) { return (int)key & kCellMax; }

__global__ __launch_bounds__(kBlock) void k_surface_rows(const unsigned long long* __restrict__ key, const long long* __restrict__ sum, const uint32_t* __restrict__ n,
                                                         const int64_t first, const int64_t count, const double cell, const float truncation, uint32_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= count) return;
    const int64_t j = first + t;
    const unsigned long long k = key[j];
    uint32_t* row = out + 5 * t;
    row[0] = __float_as_uint(occupancy_centre(d_key_x(k) - kCellBias, cell));
    row[1] = __float_as_uint(occupancy_centre(d_key_y(k) - kCellBias, cell));
    row[2] = __float_as_uint(occupancy_centre(d_key_z(k) - kCellBias, cell));
    row[3] = __float_as_uint(surface_tsdf(sum[j], n[j], truncation)), row[4] = n[j];
}

// the listing index of the cell (x, y, z) (biased), or -1 if the volume does not hold it
__device__ __forceinline__ int64_t d_surface_index(const SurfaceVolume& v, const int x, const int y, const int z) {
    if (x < 0 || x > kCellMax || y < 0 || y > kCellMax || z < 0 || z > kCellMax) return -1;
    const unsigned long long key = d_cell_key(x, y, z);
    uint32_t slot = (uint32_t)mix64(key) & v.mask;
#pragma unroll 1
    for (uint32_t probe = 0; probe <= v.mask; ++probe) {
        const unsigned long long kk = v.table[slot].key;
        if (kk == key) {
            const int64_t j = (int64_t)v.table[slot].index;
            return j < v.m ? j : -1;  // (always j < m: the listing wrote it)
        }
        if (kk == kCellEmptyKey) return -1;
        slot = (slot + 1) & v.mask;
    }
    return -1;
}

// the cube of anchor j: the listing index of every corner (by mask) in idx[8], -1 where the node is missing or not valid; the return value
// has bit m set iff corner m is valid, bit 8 + m iff it is inside.  0 if the anchor itself is not valid.
__device__ __forceinline__ uint32_t d_mesh_cube(const SurfaceVolume& v, const int64_t j, const uint32_t min_weight, int64_t idx[8]) {
#pragma unroll
    for (int m = 0; m < 8; ++m) idx[m] = -1;
    if (v.n[j] < min_weight) return 0u;
    const unsigned long long k = v.key[j];
    const int x = d_key_x(k), y = d_key_y(k), z = d_key_z(k);
    uint32_t bits = 0u;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int64_t at = m == 0 ? j : d_surface_index(v, x + (m & 1), y + (m >> 1 & 1), z + (m >> 2 & 1));
        if (at < 0 || v.n[at] < min_weight) continue;
        idx[m] = at;
        bits |= 1u << m;
        if (v.sum[at] < 0) bits |= 1u << (8 + m);
    }
    return bits;
}
// corner `mask` of the cube, picked without a dynamic index
__device__ __forceinline__ int64_t d_pick(const int64_t idx[8], const uint32_t mask) {
    int64_t at = idx[0];
#pragma unroll
    for (int m = 1; m < 8; ++m) at = mask == (uint32_t)m ? idx[m] : at;
    return at;
}
// tetrahedron t of a cube: false if one of its nodes is not valid; else *in4 = the chain positions that are inside
__device__ __forceinline__ bool d_mesh_tetra(const uint32_t bits, const uint32_t chain, uint32_t* in4) {
    uint32_t in = 0u;
    bool all = true;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint32_t mask = surface_chain_mask(chain, p);
        all = all && (bits >> mask & 1u);
        in |= (bits >> (8 + mask) & 1u) << p;
    }
    *in4 = in;
    return all;
}

__global__ __launch_bounds__(kBlock) void k_mesh_mark(const SurfaceVolume v, const uint32_t min_weight, int32_t* __restrict__ tris, uint8_t* used,
                                                      unsigned long long* __restrict__ sums) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long meshed = 0ull, made = 0ull;
    if (j < v.m) {
        int64_t idx[8];
        const uint32_t bits = d_mesh_cube(v, j, min_weight, idx);
        if (bits & 1u) {
#pragma unroll 1
            for (int t = 0; t < 6; ++t) {
                const uint32_t chain = surface_chain(t);
                uint32_t in4;
                if (!d_mesh_tetra(bits, chain, &in4)) continue;
                ++meshed;
                const uint32_t list = surface_tetra_triangles(in4);
                const uint32_t count = list >> 24;
                made += count;
                for (uint32_t c = 0; c < 3 * count; ++c) {  // (at most six corners)
                    const uint32_t e = (list >> (4 * c)) & 15u;
                    const uint32_t lo = surface_chain_mask(chain, (int)(e >> 2)), hi = surface_chain_mask(chain, (int)(e & 3u));
                    const int64_t node = d_pick(idx, lo);
                    if (node >= 0 && node < v.m) used[node * kMeshClasses + (hi & ~lo)] = (uint8_t)1;
                }
            }
        }
    }
    if (j <= v.m) tris[j] = (int32_t)made;  // (made = 0 at j = m)
    d_add_wave(meshed, sums + MW_TETRAHEDRA);
    d_add_wave(made, sums + MW_TRIANGLES);
}

// the flags of a node as one word, a byte per class
__device__ __forceinline__ unsigned long long d_used_word(const uint8_t* used, const int64_t node) {
    return reinterpret_cast<const unsigned long long*>(used)[node] & 0x0101010101010100ull;
}

__global__ __launch_bounds__(kBlock) void k_mesh_count(const uint8_t* __restrict__ used, const int64_t m, int32_t* __restrict__ verts,
                                                       unsigned long long* __restrict__ sums) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long mine = 0ull;
    if (j < m) mine = (unsigned long long)__popcll(d_used_word(used, j));
    if (j <= m) verts[j] = (int32_t)mine;
    d_add_wave(mine, sums + MW_VERTICES);
}

__global__ __launch_bounds__(kBlock) void k_mesh_emit(const SurfaceVolume v, const uint32_t min_weight, const SurfaceOrientation orient, const uint8_t* __restrict__ used,
                                                      const int32_t* __restrict__ vert_scan, const int32_t* __restrict__ tri_scan, const int64_t vertices,
                                                      const int64_t triangles, float* __restrict__ xyz, int32_t* __restrict__ indices) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= v.m) return;
    const unsigned long long k = v.key[j];
    const int x = d_key_x(k), y = d_key_y(k), z = d_key_z(k);
    // the vertices whose lower node this is, in class order
    const unsigned long long mine = d_used_word(used, j);
    if (mine != 0ull) {
        int64_t at = (int64_t)vert_scan[j];
#pragma unroll 1
        for (int cls = 1; cls < kMeshClasses; ++cls) {
            if (!(mine >> (8 * cls) & 1ull)) continue;
            const int ox = cls & 1, oy = cls >> 1 & 1, oz = cls >> 2 & 1;
            const int64_t up = d_surface_index(v, x + ox, y + oy, z + oz);
            if (up >= 0 && at >= 0 && at < vertices) {  // (always: k_mesh_mark found the upper node, the scan counted this flag)
                const double t = surface_crossing(v.sum[j], v.n[j], v.sum[up], v.n[up]);
                xyz[3 * at] = surface_vertex_axis(x - kCellBias, t, ox, v.cell);
                xyz[3 * at + 1] = surface_vertex_axis(y - kCellBias, t, oy, v.cell);
                xyz[3 * at + 2] = surface_vertex_axis(z - kCellBias, t, oz, v.cell);
            }
            ++at;
        }
    }
    // the triangles of this anchor's cube
    int64_t idx[8];
    const uint32_t bits = d_mesh_cube(v, j, min_weight, idx);
    if (!(bits & 1u)) return;
    int64_t at = (int64_t)tri_scan[j];
#pragma unroll 1
    for (int t = 0; t < 6; ++t) {
        const uint32_t chain = surface_chain(t);
        uint32_t in4;
        if (!d_mesh_tetra(bits, chain, &in4)) continue;
        const uint32_t list = surface_tetra_triangles(in4);
        for (uint32_t tri = 0; tri < (list >> 24); ++tri, ++at) {
            int32_t corner[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t e = (list >> (12 * tri + 4 * c)) & 15u;
                const uint32_t lo = surface_chain_mask(chain, (int)(e >> 2)), hi = surface_chain_mask(chain, (int)(e & 3u));
                const int64_t node = d_pick(idx, lo);
                const uint32_t cls = hi & ~lo;
                if (node < 0 || node >= v.m) {  // (never: the four nodes of a meshed tetrahedron are valid)
                    corner[c] = 0;
                    continue;
                }
                // the vertex's place: its node's first, then the flagged classes below its own
                const unsigned long long below = d_used_word(used, node) & ((1ull << (8 * cls)) - 1ull);
                corner[c] = vert_scan[node] + (int32_t)__popcll(below);
            }
            const bool flip = (orient.flip[t] >> (2 * in4 + tri)) & 1u;
            if (at >= 0 && at < triangles) indices[3 * at] = corner[0], indices[3 * at + 1] = flip ? corner[2] : corner[1], indices[3 * at + 2] = flip ? corner[1] : corner[2];
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_mesh_face_rows(const int32_t* __restrict__ indices, const int64_t first, const int64_t count, uint8_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= count) return;
    uint8_t* row = out + 13 * t;
    row[0] = (uint8_t)3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t i = (uint32_t)indices[3 * (first + t) + c];
        row[1 + 4 * c] = (uint8_t)i, row[2 + 4 * c] = (uint8_t)(i >> 8), row[3 + 4 * c] = (uint8_t)(i >> 16), row[4 + 4 * c] = (uint8_t)(i >> 24);
    }
}

}  // namespace

void launch_surface_clear(SurfaceSlot* table, uint64_t slots, hipStream_t s) {
    if (slots > 0) hipLaunchKernelGGL(k_surface_clear, dim3(blocks_for(slots)), dim3(kBlock), 0, s, table, (unsigned long long)slots);
}
void launch_surface_integrate(const GridView& grid, const float4* origin, SurfaceParams p, SurfaceSlot* table, uint32_t mask, uint64_t limit, unsigned long long* rec,
                              hipStream_t s) {
    if (grid.n > 0)
        hipLaunchKernelGGL(k_surface_integrate, dim3(blocks_for(grid.n)), dim3(kBlock), 0, s, grid.pts_sorted, grid.idx_sorted, origin, grid.n, p, table, mask,
                           (unsigned long long)limit, rec);
}
void launch_surface_flags(const SurfaceSlot* table, uint64_t slots, int32_t* flag, hipStream_t s) {
    hipLaunchKernelGGL(k_surface_flags, dim3(blocks_for(slots + 1)), dim3(kBlock), 0, s, table, (unsigned long long)slots, flag);
}
void launch_surface_compact(const SurfaceSlot* table, uint64_t slots, const int32_t* flag, const int32_t* scan, int64_t m, unsigned long long* key, uint32_t* slot_of,
                            hipStream_t s) {
    if (slots > 0) hipLaunchKernelGGL(k_surface_compact, dim3(blocks_for(slots)), dim3(kBlock), 0, s, table, (unsigned long long)slots, flag, scan, m, key, slot_of);
}
void launch_surface_list(SurfaceSlot* table, const uint32_t* slot_sorted, int64_t m, uint32_t min_weight, long long* sum, uint32_t* n, unsigned long long* rec,
                         hipStream_t s) {
    if (m > 0) hipLaunchKernelGGL(k_surface_list, dim3(blocks_for(m)), dim3(kBlock), 0, s, table, slot_sorted, m, min_weight, sum, n, rec);
}
void launch_surface_rows(const unsigned long long* key, const long long* sum, const uint32_t* n, int64_t first, int64_t count, double cell, float truncation, uint32_t* out,
                         hipStream_t s) {
    if (count > 0) hipLaunchKernelGGL(k_surface_rows, dim3(blocks_for(count)), dim3(kBlock), 0, s, key, sum, n, first, count, cell, truncation, out);
}
void launch_mesh_mark(const SurfaceVolume& v, uint32_t min_weight, int32_t* tris, uint8_t* used, unsigned long long* sums, hipStream_t s) {
    hipLaunchKernelGGL(k_mesh_mark, dim3(blocks_for((unsigned long long)v.m + 1)), dim3(kBlock), 0, s, v, min_weight, tris, used, sums);
}
void launch_mesh_count(const uint8_t* used, int64_t m, int32_t* verts, unsigned long long* sums, hipStream_t s) {
    hipLaunchKernelGGL(k_mesh_count, dim3(blocks_for((unsigned long long)m + 1)), dim3(kBlock), 0, s, used, m, verts, sums);
}
void launch_mesh_emit(const SurfaceVolume& v, uint32_t min_weight, SurfaceOrientation orient, const uint8_t* used, const int32_t* vert_scan, const int32_t* tri_scan,
                      int64_t vertices, int64_t triangles, float* xyz, int32_t* indices, hipStream_t s) {
    if (v.m > 0) hipLaunchKernelGGL(k_mesh_emit, dim3(blocks_for(v.m)), dim3(kBlock), 0, s, v, min_weight, orient, used, vert_scan, tri_scan, vertices, triangles, xyz, indices);
}
void launch_mesh_face_rows(const int32_t* indices, int64_t first, int64_t count, uint8_t* out, hipStream_t s) {
    if (count > 0) hipLaunchKernelGGL(k_mesh_face_rows, dim3(blocks_for(count)), dim3(kBlock), 0, s, indices, first, count, out);
}

}  // namespace dmsa
