// dense_cloud_obj.h — the object behind include/dmsa_dense_cloud.h, include/dmsa_dense_normals.h, include/dmsa_dense_outliers.h,
// include/dmsa_dense_carve.h, include/dmsa_dense_clusters.h and include/dmsa_dense_compare.h (and the intensity switch of include/dmsa_dense_intensity.h), shared by dense_cloud_api.cpp (scans, voxel set, the streaming file), dense_store.cpp (the retained store, the
// search grid over it, a row mask, the preconditions and the files of the store), dense_normals_api.cpp (moments, normals),
// dense_outliers_api.cpp (k-nearest-neighbour distances, the classification), dense_carve_api.cpp (the rays' walks, the pass counts) and
// dense_clusters_api.cpp (the union-find, labels and sizes, the classification by size), dense_compare_api.cpp (the reference cloud and its own
// grid, nearest rows across the two sets, the sums, the classification by distance) and dense_align_api.cpp (include/dmsa_dense_align.h and
// include/dmsa_dense_align_plane.h: the reference aligned by ICP on exact sums, point to point and point to plane) and
// dense_occupancy_api.cpp (include/dmsa_dense_occupancy.h: the occupancy map of the store's rays, its voxel file and its 2-D map) and
// dense_surface_api.cpp (include/dmsa_dense_surface.h: the signed distance field of the store's rays, its voxel file, its mesh and the PLY).
// Internal.  Both writers own a CopyBack (copy_back.h: slots, events, the reuse rule) and write through a PcdFile (pcd_file.h).
#pragma once
#include "copy_back.h"

#include <cstring>

#include "../../include/dmsa_dense_cloud.h"
#include "../../include/dmsa_dense_normals.h"
#include "../../include/dmsa_dense_outliers.h"
#include "../../include/dmsa_dense_carve.h"
#include "../../include/dmsa_dense_intensity.h"
#include "../../include/dmsa_dense_clusters.h"
#include "../../include/dmsa_dense_compare.h"
#include "../../include/dmsa_dense_align.h"
#include "../../include/dmsa_dense_align_plane.h"
#include "../../include/dmsa_dense_occupancy.h"
#include "../../include/dmsa_dense_surface.h"
#include "dense_cloud.h"
#include "dense_grid.h"

// include/dmsa_dense_normals.h, N0: the survivors of all scans and their sensor origins, float4 each, grown by doubling (empty on an object
// that does not retain).  dense_store.cpp.
struct RetainedStore {
    bool on = false;
    DevBuf g, o;
    int64_t n = 0, cap = 0;
    // room for m more rows (grown by doubling, the rows so far copied over); DMSA_ERR_NOMEM leaves the store as it was
    int reserve(dmsa_ctx* ctx, int64_t m);
    // the m rows of src_g / src_o enqueued behind the rows so far; the caller commits with n += m once the scan has succeeded
    int append(dmsa_ctx* ctx, const DevBuf& src_g, const DevBuf& src_o, int64_t m);
    // compacted to the m rows with keep[i] = 1, stably, points and origins alike (scan = the exclusive scan of keep over n + 1 flags); the caller
    // tells the stages (store_changed).  `what` opens the reason of a failure.
    int compact(dmsa_ctx* ctx, const int32_t* keep, const int32_t* scan, int64_t m, const char* what);
    int read(dmsa_ctx* ctx, int64_t first, int64_t count, float* xyz_out, float* origin_out);  // rows to the host (null: not wanted), waited for
};

// The search grid over the rows of a point set (the store's: shared.grid; the reference cloud's: compare.ref_grid): the rows sorted by cell
// (the library's stable 64-bit sort) and the cell table, kept until the set changes or another edge is asked for.  dense_store.cpp on top of
// dense_grid.hip.
struct SearchGrid {
    DevBuf key, idx, key_s, idx_s, sort_tmp, pts, table, cells;
    PinnedBuf h_cells;  // the occupied cells: the one host read of a build
    uint32_t mask = 0;
    double edge = 0.0;  // the grid is over the first `rows` rows with cells of this edge (rows = 0: none)
    int64_t rows = 0;
    // over the n rows of `points`; with `valid` (n bytes) over the n_valid rows whose byte is set, the others left out of the sort
    int build(dmsa_ctx* ctx, const float4* points, int64_t n, double edge_asked, const uint8_t* valid = nullptr, int64_t n_valid = 0);
    GridView view() const { return GridView{pts.as<float4>(), idx_s.as<uint32_t>(), key_s.as<unsigned long long>(), rows, table.as<DenseCellEntry>(), mask}; }
};
// the neighbourhood calls build the grid with this edge: cells a ball of that radius cannot cross
inline double dense_radius_edge(float radius) { return 1.001 * (double)radius; }
// e with radius = f * 2^e, 0.5 <= f < 1: the fixed-point scales of N3 and O4 are 2^(20 - e) and 2^(18 - e)
inline int dense_radius_exponent(float radius) {
    int e = 0;
    return (void)std::frexp(radius, &e), e;
}

// One classification of the store's rows: keep flags and their exclusive scan, n + 1 int32 each, and the number of rows kept.  A stage owns
// its own, so that either classification outlives the other stage's call.
struct RowMask {
    DevBuf keep, scan;
    int64_t rows = -1;  // keep / scan classify the `rows` rows of the store as it stands (-1: no valid classification)
    int64_t kept = 0;
    hipError_t begin(int64_t n);  // a classification of n rows starts: whatever fails from here on leaves none
    // enqueued: scan = the exclusive scan of keep over n + 1 flags ...
    hipError_t enqueue_scan(int64_t n, DevBuf& scan_tmp, hipStream_t s);
    // ... and scan[n], the rows kept, into a pinned word
    hipError_t enqueue_count(int64_t n, int32_t* word, hipStream_t s) { return h_kept = word, hipMemcpyAsync(word, scan.as<int32_t>() + n, 4, hipMemcpyDeviceToHost, s); }
    void commit(int64_t n) { kept = *h_kept, rows = n; }  // after the call's own final synchronisation
    bool valid_for(const RetainedStore& store) const { return store.on && rows >= 0 && rows == store.n; }

private:
    const int32_t* h_kept = nullptr;
};

// What the three stages share and what each owns; every buffer is allocated on first use and released with the object.
struct DenseShared {
    SearchGrid grid;
    CopyBack files;  // the files of the store, chunk by chunk
    DevBuf scan_tmp;
};
struct DenseNormals {
    DevBuf moments, normal, without;
    PinnedBuf h_without;  // rows without a normal
    bool valid = false;   // `normal` holds N4 of all rows of the store
};
struct DenseOutliers {
    DevBuf knn_mean, knn_q, flag8, sums;  // m_i, q_i, the flags as bytes for the caller, the sums of O4
    PinnedBuf h_sums;                     // OS_COUNT words, then the number of inliers (int32)
    RowMask mask;
};
struct DenseCarve {
    DevBuf passes, walk_cells, walk_hash, sums;  // passes_j, the stage call's outputs, the sums of T6
    PinnedBuf h_sums;                            // CS_COUNT words, then the number of rows kept (int32)
    RowMask mask;
};

struct DenseClusters {
    DevBuf parent, root, min_row, count;  // the union-find over the sorted rows, every row's root, per root the smallest store row and its rows
    DevBuf label, size, flag8, sums;      // C3 per store row, the flags as bytes for the caller, the sums of C5 and the give-up word
    PinnedBuf h_sums;                     // CL_COUNT words, then the number of rows kept (int32)
    RowMask mask;
    int64_t label_rows = -1;              // label / size are C3 of the `label_rows` rows of the store as it stands at ... (-1: no valid labels)
    float label_radius = 0.0f;            // ... this radius
    bool labels_valid_for(const RetainedStore& store) const { return store.on && label_rows >= 0 && label_rows == store.n; }
};

// include/dmsa_dense_compare.h.  The reference belongs to the object, not to the store: store_changed leaves ref, ref_valid and ref_grid alone.
struct DenseCompare {
    DevBuf ref, ref_valid;  // D0: the transformed rows (float4, w = 0) and their validity bytes
    int64_t ref_rows = 0, ref_valid_rows = 0;
    SearchGrid ref_grid;    // over the valid rows
    // per direction (0: accuracy, the store's rows as queries; 1: completeness, the reference's): D2's keys, dist and index
    DevBuf best[2], dist[2], index[2];
    DevBuf flag8, sums;     // the flags as bytes for the caller; two blocks of CM_COUNT words
    PinnedBuf h_sums;       // the two blocks, then the number of rows kept (int32)
    RowMask mask;
    int64_t dist_rows = -1;  // best[0] / dist[0] are D2 of the `dist_rows` rows of the store as it stands against the reference as it stands
    bool distances_valid_for(const RetainedStore& store) const { return store.on && dist_rows >= 0 && dist_rows == store.n; }
};

// include/dmsa_dense_align.h and include/dmsa_dense_align_plane.h.  The pairs of an iteration are the completeness direction's
// (compare.best[1], dist[1], index[1]); this stage owns only the way its sums reach the host: ONE slot (0) of a CopyBack for both metrics,
// the metric's own words (kAlignSums of A2 or kAlignPlaneSums of P2) and then one block of CM_COUNT words of D4.  Every call waits for its
// copy before it returns, so no two blocks are ever on their way.  Nothing here is allocated or created before the first alignment call.
struct DenseAlign {
    CopyBack back;
    bool created = false;
};

// include/dmsa_dense_occupancy.h.  The table of a build, the listing of M4 (keys, counters and states side by side, `cells` entries) and the
// buffers of the two products; dense_occupancy_api.cpp.
struct DenseOccupancy {
    DevBuf table, rec, flag, scan, key, slot_of, key_s, slot_s, sort_tmp;  // the walk's table and record; the held slots compacted and sorted
    DevBuf hits, passes, state, sums;                                      // the listing beside key_s; the sums of the listing and of a slice
    DevBuf keep, keep_scan, sel;                                           // M6: the listed cells a file takes
    DevBuf extent, image, pixels;                                          // M7
    PinnedBuf h_rec;      // OW_COUNT words, then OS_STATES words, then four int32 of an extent and one of a count
    int64_t rows = -1;    // the map is of the `rows` rows of the store as it stands (-1: no valid map)
    int64_t cells = 0;    // of the listing
    float cell_size = 0;  // the config's, as given
    bool valid_for(const RetainedStore& store) const { return store.on && rows >= 0 && rows == store.n; }
};

// include/dmsa_dense_surface.h.  The table of a build, the listing of S6 (keys, sums and weights side by side, `cells` entries; the table
// stays, with every cell's listing index in its slot) and the mesh of S8; dense_surface_api.cpp.
struct DenseSurface {
    DevBuf table, rec, flag, scan, key, slot_of, key_s, slot_s, sort_tmp;  // the walk's table and record; the held slots compacted and sorted
    DevBuf sum, weight;                                                    // the listing beside key_s
    DevBuf used, tris, verts, tri_scan, vert_scan, sums, xyz, indices;     // S8: flags and counts, their scans, the mesh
    PinnedBuf h_rec;            // SW_COUNT words, then MW_COUNT words
    int64_t rows = -1;          // the volume is of the `rows` rows of the store as it stands (-1: no valid volume)
    int64_t cells = 0;          // of the listing
    uint64_t slots = 0;         // of the table the listing's indices live in
    float cell_size = 0, truncation = 0;  // the config's, as given
    int64_t vertices = -1, triangles = 0;  // the mesh of this volume (-1: none extracted)
    bool valid_for(const RetainedStore& store) const { return store.on && rows >= 0 && rows == store.n; }
    bool mesh_valid_for(const RetainedStore& store) const { return valid_for(store) && vertices >= 0; }
};

struct dmsa_dense_cloud {
    dmsa_ctx* ctx = nullptr;
    dmsa_dense_config cfg{};
    DenseGates gates{};
    int64_t n_p = 0;
    bool intensity = false;  // include/dmsa_dense_intensity.h, I1: the fourth float of a point row is its intensity, and the files have the field
    int point_floats() const { return intensity ? 4 : 3; }  // floats of a point in a file row
    DevBuf d_stamps, d_pos, d_quat;  // the trajectory (quaternions as w, x, y, z)
    // one scan
    DevBuf d_raw, d_xyz, d_stamp, d_id, d_placed, d_keep, d_scan, d_key, d_slot, d_out, d_counters, d_scan_tmp, d_pose12, d_seg;
    // the voxel set
    DevBuf table;
    uint64_t slots = 0;    // a power of two, or 0 before the first scan
    int64_t occupied = 0;  // voxels entered so far (= points kept so far)
    uint32_t scan_no = 0;
    dmsa_dense_stats total{};
    struct Readback {
        unsigned long long counters[DC_COUNT];
        int32_t kept;
    };
    PinnedBuf h_rb;
    Readback* rb() const { return h_rb.as<Readback>(); }
    // the file
    PcdFile file;
    int64_t file_points = 0;
    CopyBack rows;                         // the copy-back of scan i runs beside the kernels of scan i + 1, its fwrite too
    int pending_slot = -1, next_slot = 0;  // the scan whose rows are on their way back and not yet written
    size_t pending_bytes = 0;
    RetainedStore store;
    DevBuf d_origin, d_out_o;  // one scan: the origin of every point, and of the survivors
    DenseShared shared;
    DenseNormals normals;
    DenseOutliers outliers;
    DenseCarve carve;
    DenseClusters clusters;
    DenseCompare compare;
    DenseAlign align;
    DenseOccupancy occupancy;
    DenseSurface surface;
};

// a scan was added or the store compacted: grid, normals, labels, the distances to the reference, the four classifications, the occupancy
// map and the surface (volume and mesh) are stale
// (the reference itself and its grid are not: include/dmsa_dense_compare.h, D0)
inline void store_changed(dmsa_dense_cloud* dc) {
    dc->shared.grid.rows = 0, dc->normals.valid = false, dc->outliers.mask.rows = -1, dc->carve.mask.rows = -1;
    dc->clusters.mask.rows = -1, dc->clusters.label_rows = -1;
    dc->compare.mask.rows = -1, dc->compare.dist_rows = -1;
    dc->occupancy.rows = -1;
    dc->surface.rows = -1, dc->surface.vertices = -1;
}

// ---- dense_compare_text.cpp ----
// what D1 asks of tolerance and keep: the reason of the first breach, or nullptr
const char* dense_compare_config_refusal(const dmsa_dense_compare_config* cfg);

// ---- dense_compare_api.cpp ----
// D0 from rows that are on the device already: n >= 1 rows of `stride_floats` floats at d_raw transformed with T (12 finite doubles, cast to
// float; null: the rows as they are) into compare.ref, their validity and the counts, waited for.  Whatever fails leaves no reference; results
// against the old one are stale either way.  dmsa_dense_cloud_set_reference and every iteration of include/dmsa_dense_align.h (A1, A7).
int dense_reference_from_device_rows(dmsa_dense_cloud* dc, const float* d_raw, int64_t n, int32_t stride_floats, const double* T);
// What the comparison and both alignments (dense_align_api.cpp) share; `what` ("dense compare", "dense align", "dense align plane") opens
// the reason of a refusal.
constexpr int64_t kMaxReference = (int64_t)1 << 26;  // D0
inline uint32_t float_bits(float v) {
    uint32_t b;
    return std::memcpy(&b, &v, 4), b;
}
// no reference; the results against the old one are stale
void dense_drop_reference(dmsa_dense_cloud* dc);
// D0 of the caller's rows: at least `least` of them (0 or 1; `too_few` is the reason otherwise), a pointer, stride_floats >= 3, at most 2^26
int dense_reference_rows_accepted(dmsa_dense_cloud* dc, const float* xyz, int64_t n, int32_t stride_floats, int64_t least, const char* too_few, const char* what);
// the n >= 1 accepted rows as they came, enqueued into `raw`; the caller keeps `raw` and xyz alive until the stream has passed the copy
int dense_upload_reference_rows(dmsa_dense_cloud* dc, const float* xyz, int64_t n, int32_t stride_floats, DevBuf* raw);
// THE PAIR PASS, D2-D4 of one direction (0: the store's rows are the queries; 1: the reference's) enqueued for the queries
// [first, first + count) of its query set: both grids built with one edge for `reach`, compare.best / dist / index [dir] hold `count`
// entries, and the CM_COUNT words at `sums` (device, zeroed by the caller) have this range's share added, `within` counted against the bits
// of a squared threshold.  A reference without a valid row has no grid and no pair: every query stays unmatched.
int dense_enqueue_pairs(dmsa_dense_cloud* dc, int dir, int64_t first, int64_t count, float reach, uint32_t within_bits, unsigned long long* sums);
// a direction's block as read back, and D5 of it with D4's scale
int dense_fill_direction(dmsa_dense_cloud* dc, const unsigned long long* h, int64_t queries, double scale, const char* what, dmsa_dense_compare_direction* d);

// ---- dense_clusters_text.cpp ----
// what C1 asks of min_size and max_size: the reason of the first breach, or nullptr
const char* dense_cluster_config_refusal(const dmsa_dense_cluster_config* cfg);

// ---- dense_carve_text.cpp ----
// what T1 asks of the config alone, cell_size apart (that one is measured against the voxel): the reason of the first breach, or nullptr
const char* dense_carve_config_refusal(const dmsa_dense_carve_config* cfg);

// ---- dense_occupancy_text.cpp ----
// what M1 asks of the config alone, cell_size apart: the reason of the first breach, or nullptr
const char* dense_occupancy_config_refusal(const dmsa_dense_occupancy_config* cfg);

// ---- dense_surface_text.cpp ----
// what S1 asks of the config alone, cell_size against the voxel apart, and of a min_weight: the reason of the first breach, or nullptr
const char* dense_surface_config_refusal(const dmsa_dense_surface_config* cfg);
const char* dense_surface_weight_refusal(int32_t min_weight);

// ---- dense_store.cpp ----
// The preconditions, each stated once; `what` ("dense normals", "dense outliers", "dense carve") opens the reason.
int dense_retention_on(dmsa_dense_cloud* dc, const char* what);
int dense_store_ready(dmsa_dense_cloud* dc, const char* what);  // retention on, at least one row, voxel_size > 0
// `x` (`name` in the reason: "radius", "cell_size") is finite and lies in [voxel_size, 64 * voxel_size]
int dense_voxel_length(dmsa_dense_cloud* dc, float x, const char* name, const char* what);
int dense_row_range(dmsa_dense_cloud* dc, int64_t first, int64_t count, const char* what);  // [first, first + count) lies in the store
int dense_row_cap(dmsa_dense_cloud* dc, const char* what);                                  // at most 2^26 rows
int dense_radius_preconditions(dmsa_dense_cloud* dc, float radius, const char* what);       // N1: the store's state, the length, the scale of N3
int dense_reach_preconditions(dmsa_dense_cloud* dc, float r, const char* name, const char* what);  // N1 of a length of another name (D1: max_distance)
// O6, T7: the store compacted by `mask` if that is of the store as it stands, `refusal` otherwise; *kept (may be null) = the rows of the store
int dense_remove_rows(dmsa_dense_cloud* dc, const RowMask& mask, const char* refusal, const char* what, int64_t* kept);
// the store as a binary PCD at `path`: rows of 3 floats (x y z), 4 (x y z intensity), 7 (x y z and normals.normal) or 8 (x y z intensity and
// normals.normal: include/dmsa_dense_intensity.h, I7), in chunks of 2^20 rows packed on the library
// stream and written through shared.files (copy_back_chunks); a failure leaves no partial file.  `word` (row_floats 3 or 4 only): one more
// word per row from a buffer of the store's rows, clusters.label (include/dmsa_dense_clusters.h, C7) or compare.dist[0]
// (include/dmsa_dense_compare.h, D7) as it stands; the header follows
enum class RowWord { none, label, distance };
int dense_save_rows(dmsa_dense_cloud* dc, const char* path, const char* what, int row_floats, int64_t* points_out, int64_t* bytes_out, RowWord word = RowWord::none);
