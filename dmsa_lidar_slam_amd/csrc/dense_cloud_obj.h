// dense_cloud_obj.h — the object behind include/dmsa_dense_cloud.h, include/dmsa_dense_normals.h, include/dmsa_dense_outliers.h and
// include/dmsa_dense_carve.h, shared by dense_cloud_api.cpp (scans, voxel set, the streaming file), dense_normals_api.cpp (the retained store,
// the search grid, normals, the files of the store, the compaction of the store), dense_outliers_api.cpp (k-nearest-neighbour distances, the
// classification) and dense_carve_api.cpp (the rays' walks, the pass counts).  Internal.
// Both writers own a CopyBack (copy_back.h: slots, events, the reuse rule) and write through a PcdFile (pcd_file.h: the file, its error texts).
#pragma once
#include "copy_back.h"

#include "../../include/dmsa_dense_cloud.h"
#include "../../include/dmsa_dense_normals.h"
#include "../../include/dmsa_dense_outliers.h"
#include "../../include/dmsa_dense_carve.h"
#include "dense_cloud.h"

struct dmsa_dense_cloud {
    dmsa_ctx* ctx = nullptr;
    dmsa_dense_config cfg{};
    DenseGates gates{};
    int64_t n_p = 0;
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
    // include/dmsa_dense_normals.h, N0: the survivors of all scans and their sensor origins, float4 each, grown by doubling (null / 0 on an
    // object that does not retain)
    bool retain = false;
    DevBuf ret_g, ret_o;
    int64_t ret_n = 0, ret_cap = 0;
    DevBuf d_origin, d_out_o;                 // one scan: the origin of every point, and of the survivors
    struct DenseNormalsState* nrm = nullptr;  // the search grid over the store and what was computed over it, created on first use
};

// the search grid, scratch and results of the normals, of the outlier classification and of the ray carving; allocated on first use
struct DenseNormalsState {
    DevBuf key, idx, key_s, idx_s, sort_tmp, pts, table, moments, normal, counter;
    uint32_t mask = 0;
    double grid_edge = 0.0;  // the grid in key_s / idx_s / pts / table is over the first grid_n rows with cells of this edge (grid_n = 0: none)
    int64_t grid_n = 0;
    bool normals_valid = false;  // `normal` holds N4 of all ret_n rows
    PinnedBuf h_counter;         // two words: occupied cells, rows without a normal
    CopyBack rows;               // the files of the store, chunk by chunk
    // include/dmsa_dense_outliers.h: m_i, q_i, the flags (int32 for the scan, bytes for the caller), their exclusive scan, the sums of O4
    DevBuf knn_mean, knn_q, keep, keep_scan, flag8, scan_tmp, sums;
    PinnedBuf h_sums;      // OS_COUNT words, then the number of inliers (int32)
    int64_t flags_n = -1;  // keep / keep_scan classify the flags_n rows of the store as it stands (-1: no valid classification)
    // include/dmsa_dense_carve.h: passes_j, the flags and their scan (its own, so that either classification outlives the other's call), the
    // stage call's outputs, the sums of T6
    DevBuf passes, carve_keep, carve_scan, walk_cells, walk_hash, carve_sums;
    PinnedBuf h_carve;     // CS_COUNT words, then the number of rows kept (int32)
    int64_t carve_n = -1;  // carve_keep / carve_scan classify the carve_n rows of the store as it stands (-1: no valid count)
};

// ---- dense_carve_text.cpp ----
// what T1 asks of the config alone, cell_size apart (that one is measured against the voxel): the reason of the first breach, or nullptr
const char* dense_carve_config_refusal(const dmsa_dense_carve_config* cfg);

// ---- dense_normals_api.cpp ----
// room for m more rows in the store (grown by doubling, the rows so far copied over); DMSA_ERR_NOMEM leaves the store as it was
int dense_retain_reserve(dmsa_dense_cloud* dc, int64_t m);
// the m survivors in d_out / d_out_o enqueued behind the rows so far; the caller commits with ret_n += m once the scan has succeeded
int dense_retain_append(dmsa_dense_cloud* dc, int64_t m);
void dense_normals_invalidate(dmsa_dense_cloud* dc);  // a scan was added or the store compacted: grid, normals and classification are stale
void dense_normals_release(dmsa_dense_cloud* dc);     // deletes dc->nrm (dmsa_dense_cloud_destroy)
int dense_normals_state(dmsa_dense_cloud* dc, DenseNormalsState** out);  // dc->nrm, created on first use
// what N1 asks of the store and of `radius`; `what` ("dense normals", "dense outliers") opens the reason
int dense_radius_preconditions(dmsa_dense_cloud* dc, float radius, const char* what);
// the search grid over all retained rows with cells of this edge (kept until the store changes or another edge is asked for); the
// neighbourhood calls pass dense_radius_edge(radius), whose cells a ball of that radius cannot cross
int dense_normals_grid(dmsa_dense_cloud* dc, DenseNormalsState* st, double edge);
inline double dense_radius_edge(float radius) { return 1.001 * (double)radius; }
// the store compacted to the m rows with keep[i] = 1, stably, points and origins alike (keep_scan = the exclusive scan of keep over n + 1
// flags); grid, normals and both classifications are invalid afterwards (O6, T7).  `what` opens the reason of a failure.
int dense_compact_store(dmsa_dense_cloud* dc, const int32_t* keep, const int32_t* keep_scan, int64_t m, const char* what);
// the store as a binary PCD at `path`: rows of 7 floats (x y z and st->normal) or of 3 (x y z), in chunks of 2^20 rows packed on the library
// stream and written through st->rows (copy_back_chunks); a failure leaves no partial file
int dense_save_rows(dmsa_dense_cloud* dc, DenseNormalsState* st, const char* path, const char* what, int row_floats, int64_t* points_out, int64_t* bytes_out);
