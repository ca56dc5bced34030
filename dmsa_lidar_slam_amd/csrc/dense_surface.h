// dense_surface.h — launchers of the kernels behind include/dmsa_dense_surface.h (csrc/dense_surface.hip): every retained ray's segment
// around its endpoint walked with csrc/dense_carve_walk.h into a table of {cell key, sum, n, listing index} (S2-S5), the table's cells listed
// in key order (S6), the rows of the voxel file (S7), the marching tetrahedra (S8) and the face rows of the mesh file (S9).  Scan and sort are
// the library's own (device_prims.h).
#pragma once
#include "dense_grid.h"
#include "dense_surface_rule.h"

namespace dmsa {

// the table of S5: DenseCellEntry's scheme (open addressing, linear probing, an all-ones key = empty); `index` is written by the listing
struct SurfaceSlot {
    unsigned long long key;  // three biased 21-bit cells, as d_cell_key builds it
    unsigned long long sum;  // the int64 sum of q, two's complement
    uint32_t n, index;       // samples; the cell's place in S6's listing
};
// the scalars of dmsa_dense_surface_config the kernels read
struct SurfaceParams {
    double cell;  // (double)cell_size
    float truncation, max_length;
};
// the record of a walk in HBM, zeroed before k_surface_integrate: the one small read of a build
enum SurfaceWord { SW_OVERFLOW = 0, SW_OCCUPIED, SW_SKIPPED, SW_CELLS, SW_OUT_OF_RANGE, SW_VALID, SW_COUNT };
// the sums of an extraction
enum MeshWord { MW_TETRAHEDRA = 0, MW_VERTICES, MW_TRIANGLES, MW_COUNT };
// the listing as the mesh kernels read it: m cells; the table finds a cell's index by its key
struct SurfaceVolume {
    const unsigned long long* key;  // sorted
    const long long* sum;
    const uint32_t* n;
    int64_t m;
    const SurfaceSlot* table;
    uint32_t mask;
    double cell;  // (double)cell_size
};
constexpr int kMeshClasses = 8;  // flag bytes per node: class 1 .. 7 (byte 0 unused), read as one 64-bit word

// every slot empty, sum and n 0
void launch_surface_clear(SurfaceSlot* table, uint64_t slots, hipStream_t s);
// S2-S5 for all rows of the grid, a ray per lane in sorted order; rec[SW_*] += this launch's share.  A table with more than `limit` keys, or a
// probe that runs out of slots, sets rec[SW_OVERFLOW]: the sums are then incomplete and the caller walks again into a larger table.
void launch_surface_integrate(const GridView& grid, const float4* origin, SurfaceParams p, SurfaceSlot* table, uint32_t mask, uint64_t limit, unsigned long long* rec,
                              hipStream_t s);
// flag[i] = slot i holds a key, for i < slots; flag[slots] = 0
void launch_surface_flags(const SurfaceSlot* table, uint64_t slots, int32_t* flag, hipStream_t s);
// key[scan[i]] = slot i's key, slot_of[scan[i]] = i for every slot that holds one (m of them: the room in key and slot_of)
void launch_surface_compact(const SurfaceSlot* table, uint64_t slots, const int32_t* flag, const int32_t* scan, int64_t m, unsigned long long* key, uint32_t* slot_of,
                            hipStream_t s);
// per listed cell j (m of them, slot_sorted[j] its slot): sum, n, and j into the slot's index; rec[SW_VALID] += cells with n >= min_weight
void launch_surface_list(SurfaceSlot* table, const uint32_t* slot_sorted, int64_t m, uint32_t min_weight, long long* sum, uint32_t* n, unsigned long long* rec, hipStream_t s);
// S7: `count` rows of 20 bytes for the listed cells first .. first + count
void launch_surface_rows(const unsigned long long* key, const long long* sum, const uint32_t* n, int64_t first, int64_t count, double cell, float truncation, uint32_t* out,
                         hipStream_t s);
// S8, an anchor per lane: tris[j] = triangles of anchor j's cube (tris[m] = 0), used[8 j + class] = 1 for every vertex a triangle refers to
// (zeroed by the caller), sums[MW_TETRAHEDRA] and sums[MW_TRIANGLES] += this launch's share
void launch_mesh_mark(const SurfaceVolume& v, uint32_t min_weight, int32_t* tris, uint8_t* used, unsigned long long* sums, hipStream_t s);
// verts[j] = vertices whose lower node is j (verts[m] = 0); sums[MW_VERTICES] += their number
void launch_mesh_count(const uint8_t* used, int64_t m, int32_t* verts, unsigned long long* sums, hipStream_t s);
// S8: the vertices of every node at vert_scan[node] on, the triangles of every anchor at tri_scan[anchor] on (room for `vertices` and
// `triangles`: nothing is written beyond)
void launch_mesh_emit(const SurfaceVolume& v, uint32_t min_weight, SurfaceOrientation orient, const uint8_t* used, const int32_t* vert_scan, const int32_t* tri_scan,
                      int64_t vertices, int64_t triangles, float* xyz, int32_t* indices, hipStream_t s);
// S9: `count` face rows of 13 bytes for the triangles first .. first + count
void launch_mesh_face_rows(const int32_t* indices, int64_t first, int64_t count, uint8_t* out, hipStream_t s);

}  // namespace dmsa
