// dense_cloud_obj.h — the object behind include/dmsa_dense_cloud.h and include/dmsa_dense_normals.h, shared by dense_cloud_api.cpp (scans, voxel
// set, the streaming file) and dense_normals_api.cpp (the retained store, neighbourhoods, normals and their file).  Internal.
#pragma once
#include "dmsa_ctx.h"

#include "../../include/dmsa_dense_cloud.h"
#include "../../include/dmsa_dense_normals.h"
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
    std::FILE* file = nullptr;
    std::string path;
    int64_t file_points = 0, file_bytes = 0;
    DevBuf d_rows[2];
    PinnedBuf h_rows[2];  // the copy-back of scan i runs beside the kernels of scan i + 1, its fwrite too
    hipEvent_t ev_pack[2] = {nullptr, nullptr}, ev_copy[2] = {nullptr, nullptr};
    int pending_slot = -1, next_slot = 0;  // the scan whose rows are on their way back and not yet written
    size_t pending_bytes = 0;
    // include/dmsa_dense_normals.h, N0: the survivors of all scans and their sensor origins, float4 each, grown by doubling (null / 0 on an
    // object that does not retain)
    bool retain = false;
    DevBuf ret_g, ret_o;
    int64_t ret_n = 0, ret_cap = 0;
    DevBuf d_origin, d_out_o;                 // one scan: the origin of every point, and of the survivors
    struct DenseNormalsState* nrm = nullptr;  // scratch and results of the normals (dense_normals_api.cpp), created on first use
};

// ---- dense_normals_api.cpp ----
// room for m more rows in the store (grown by doubling, the rows so far copied over); DMSA_ERR_NOMEM leaves the store as it was
int dense_retain_reserve(dmsa_dense_cloud* dc, int64_t m);
// the m survivors in d_out / d_out_o enqueued behind the rows so far; the caller commits with ret_n += m once the scan has succeeded
int dense_retain_append(dmsa_dense_cloud* dc, int64_t m);
void dense_normals_invalidate(dmsa_dense_cloud* dc);  // a scan was added: grid and normals are stale
void dense_normals_release(dmsa_dense_cloud* dc);     // deletes dc->nrm (dmsa_dense_cloud_destroy)
