// dense_cloud_api.cpp — include/dmsa_dense_cloud.h on top of dense_cloud.hip: the trajectory upload, the launch sequence of a scan, the voxel
// table's growth, and the binary PCD written scan by scan (a scan's rows come back through copy_back.h while the next scan runs, and go into a
// pcd_file.h).  The TUM parser and the file's header are host-only code of their own: dense_cloud_text.cpp.
#include "dense_cloud_obj.h"

namespace {

constexpr uint64_t kMaxSlots = (uint64_t)1 << 30;  // 16 GiB of table; a slot index fits the int32 the kernels remember per point
constexpr int64_t kMaxScanPoints = 0x7FFFFFF0;

DenseTraj traj_of(const dmsa_dense_cloud* dc) { return DenseTraj{dc->d_stamps.as<double>(), dc->d_pos.as<double>(), dc->d_quat.as<double>(), (int32_t)dc->n_p}; }

// the table holds `n` more points at no more than half full: grown to the next power of two and rehashed on the device otherwise
int ensure_table(dmsa_dense_cloud* dc, int64_t n) {
    dmsa_ctx* ctx = dc->ctx;
    const uint64_t need = 2 * ((uint64_t)dc->occupied + (uint64_t)n);
    if (need <= dc->slots) return DMSA_OK;
    uint64_t slots = 1024;
    while (slots < need) slots <<= 1;
    if (slots > kMaxSlots) return fail(ctx, DMSA_ERR_NOMEM, "dense cloud: the voxel table would exceed 2^30 slots");
    DevBuf grown;
    if (grown.ensure((size_t)slots * sizeof(VoxelSlot)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, DMSA_ERR_NOMEM, "dense cloud: no device memory for a voxel table of " + std::to_string(slots) + " slots");
    }
    launch_voxel_clear(grown.as<VoxelSlot>(), slots, ctx->stream);
    if (dc->slots > 0) {
        HIPCHK(dc->d_counters.ensure(DC_COUNT * 8));
        HIPCHK(hipMemsetAsync(dc->d_counters.p, 0, DC_COUNT * 8, ctx->stream));
        launch_voxel_rehash(dc->table.as<VoxelSlot>(), dc->slots, grown.as<VoxelSlot>(), slots - 1, dc->d_counters.as<unsigned long long>(), ctx->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(dc->rb()->counters, dc->d_counters.p, DC_COUNT * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (dc->slots > 0 && dc->rb()->counters[DC_PROBE_FAILED] != 0) return fail(ctx, DMSA_ERR_NOMEM, "dense cloud: rehash: a probe ran out of its bound");
    dc->table.swap(grown);
    dc->slots = slots;
    return DMSA_OK;  // (`grown` frees the old table)
}

// the rows of the scan before, copied back on stream2 since: wait for them and write them
int flush_pending(dmsa_dense_cloud* dc) {
    dmsa_ctx* ctx = dc->ctx;
    if (dc->pending_slot < 0) return DMSA_OK;
    const int b = dc->pending_slot;
    dc->pending_slot = -1;
    const void* rows = nullptr;
    HIPCHK(dc->rows.wait_copied(b, &rows));
    if (!dc->file.is_open()) return DMSA_OK;
    if (!dc->file.write(rows, dc->pending_bytes)) return fail(ctx, DMSA_ERR_INVALID, dc->file.why());
    dc->file_points += (int64_t)(dc->pending_bytes / ((size_t)dc->point_floats() * 4));
    return DMSA_OK;
}

// rules 1-7 for the n points in d_xyz / d_stamp
int run_scan(dmsa_dense_cloud* dc, int64_t n, float* xyz_out, int64_t cap, int64_t* kept, dmsa_dense_stats* call_stats) {
    dmsa_ctx* ctx = dc->ctx;
    dmsa_dense_stats st{};
    st.points_in = n;
    *kept = 0;
    if (call_stats) *call_stats = st;
    if (n == 0) return DMSA_OK;
    const bool voxel = dc->cfg.voxel_size > 0.0f;
    const size_t un = (size_t)n;
    HIPCHK(dc->d_placed.ensure(un * 16));
    HIPCHK(dc->d_keep.ensure((un + 1) * 4));
    HIPCHK(dc->d_scan.ensure((un + 1) * 4));
    HIPCHK(dc->d_key.ensure(un * 8));
    HIPCHK(dc->d_slot.ensure(un * 4));
    HIPCHK(dc->d_counters.ensure(DC_COUNT * 8));
    HIPCHK(dc->d_scan_tmp.ensure(scan_temp_bytes(un + 1)));
    if (dc->store.on) HIPCHK(dc->d_origin.ensure(un * 16));
    if (voxel) CHK(ensure_table(dc, n));
    unsigned long long* counters = dc->d_counters.as<unsigned long long>();
    int32_t* keep = dc->d_keep.as<int32_t>();
    HIPCHK(hipMemsetAsync(counters, 0, DC_COUNT * 8, ctx->stream));
    launch_dense_place(dc->d_xyz.as<float4>(), dc->d_stamp.as<double>(), n, traj_of(dc), dc->gates, dc->d_placed.as<float4>(), keep,
                       dc->d_key.as<unsigned long long>(), counters, dc->store.on ? dc->d_origin.as<float4>() : nullptr, dc->intensity, ctx->stream);
    if (voxel) {
        launch_voxel_claim(keep, dc->d_key.as<unsigned long long>(), n, dc->scan_no, dc->table.as<VoxelSlot>(), dc->slots - 1, dc->d_slot.as<int32_t>(), counters,
                           ctx->stream);
        launch_voxel_resolve(keep, dc->d_slot.as<int32_t>(), n, dc->scan_no, dc->table.as<VoxelSlot>(), counters, ctx->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(exclusive_scan_i32(dc->d_scan_tmp.p, dc->d_scan_tmp.cap, keep, dc->d_scan.as<int32_t>(), un + 1, ctx->stream));
    HIPCHK(hipMemcpyAsync(dc->rb()->counters, counters, DC_COUNT * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&dc->rb()->kept, dc->d_scan.as<int32_t>() + n, 4, hipMemcpyDeviceToHost, ctx->stream));
    // the host writes the rows of the scan before while the device works on this one
    const int wrc = flush_pending(dc);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    // whatever fails from here on takes the scan out of the voxel set again
    auto undo = [&](int rc) -> int {
        if (voxel) {
            launch_voxel_rollback(keep, dc->d_slot.as<int32_t>(), n, dc->table.as<VoxelSlot>(), ctx->stream);
            (void)hipStreamSynchronize(ctx->stream);
        }
        return rc;
    };
    if (wrc != DMSA_OK) return undo(wrc);
    const unsigned long long* c = dc->rb()->counters;
    const int64_t m = dc->rb()->kept;
    st.kept = m, st.non_finite = (int64_t)c[DC_NON_FINITE], st.out_of_range = (int64_t)c[DC_OUT_OF_RANGE], st.out_of_time = (int64_t)c[DC_OUT_OF_TIME];
    st.in_gap = (int64_t)c[DC_IN_GAP], st.out_of_grid = (int64_t)c[DC_OUT_OF_GRID], st.thinned = (int64_t)c[DC_THINNED];
    if (c[DC_PROBE_FAILED] != 0) return undo(fail(ctx, DMSA_ERR_NOMEM, "dense cloud: voxel table: a probe ran out of its bound"));
    *kept = m;
    if (call_stats) *call_stats = st;
    if (xyz_out && m > cap) return undo(fail(ctx, DMSA_ERR_INVALID, "dense cloud: capacity too small (*kept holds the points of the scan)"));
    if (dc->store.on && m > 0) {
        const int rrc = dc->store.reserve(ctx, m);
        if (rrc != DMSA_OK) return undo(rrc);
    }
    if (m > 0) {
        HIPCHK(dc->d_out.ensure((size_t)m * 16));
        launch_dense_scatter(dc->d_placed.as<float4>(), keep, dc->d_scan.as<int32_t>(), n, dc->d_out.as<float4>(), ctx->stream);
        HIPCHK(hipGetLastError());
        if (dc->store.on) {
            HIPCHK(dc->d_out_o.ensure((size_t)m * 16));
            launch_dense_scatter(dc->d_origin.as<float4>(), keep, dc->d_scan.as<int32_t>(), n, dc->d_out_o.as<float4>(), ctx->stream);
            HIPCHK(hipGetLastError());
            CHK(dc->store.append(ctx, dc->d_out, dc->d_out_o, m));
        }
        if (xyz_out) HIPCHK(hipMemcpyAsync(xyz_out, dc->d_out.p, (size_t)m * 16, hipMemcpyDeviceToHost, ctx->stream));
        if (dc->file.is_open()) {
            const int b = dc->next_slot;
            const size_t bytes = (size_t)m * (size_t)dc->point_floats() * 4;
            HIPCHK(dc->rows.reserve(b, bytes, bytes, bytes + bytes / 4));  // (flush_pending waited for the slot's earlier copy and wrote the one before)
            launch_dense_pack_rows(dc->d_out.as<float4>(), nullptr, m, dc->point_floats(), dc->rows.dev[b].as<float>(), ctx->stream);
            HIPCHK(hipGetLastError());
            HIPCHK(dc->rows.produced(b, ctx->stream));
            HIPCHK(dc->rows.copy_back(b, bytes, ctx->stream2));
            dc->pending_slot = b, dc->pending_bytes = bytes, dc->next_slot = b ^ 1;
        }
        // d_out is scattered into again by the next scan: this scan's readers are done with it when the library stream is idle
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    if (voxel) dc->occupied += m;
    if (dc->store.on) dc->store.n += m, store_changed(dc);  // the commit point: a refused scan left the store as it was
    ++dc->scan_no;
    dmsa_dense_stats& t = dc->total;
    t.points_in += st.points_in, t.kept += st.kept, t.non_finite += st.non_finite, t.out_of_range += st.out_of_range, t.out_of_time += st.out_of_time;
    t.in_gap += st.in_gap, t.out_of_grid += st.out_of_grid, t.thinned += st.thinned;
    return DMSA_OK;
}

// the header of the streaming file: x y z, or x y z intensity (include/dmsa_dense_intensity.h, I7)
int file_header(const dmsa_dense_cloud* dc, int64_t n, char* out, int32_t cap) {
    return dc->intensity ? dmsa_pcd_header_xyzi_binary(n, out, cap) : dmsa_pcd_header_xyz_binary(n, out, cap);
}

// one message into d_raw, decoded into d_xyz / d_stamp / d_id; `field` (may be null): its values into the fourth float of d_xyz (I5)
int decode_message(dmsa_dense_cloud* dc, const dmsa_pointcloud2* msg, int32_t sensor, const dmsa_pointcloud2_field* field, size_t* n_out) {
    dmsa_ctx* ctx = dc->ctx;
    uint64_t n64 = 0;
    uint32_t field_offset = 0;
    PointCloud2Fields f{};
    CHK(pointcloud2_layout(msg, sensor, &f, &n64));
    if (field && n64 > 0) CHK(pointcloud2_field_layout(msg, field->index, field->datatype, &field_offset));
    CHK(set_device(ctx));
    const size_t n = (size_t)n64;
    *n_out = n;
    if (n == 0) return DMSA_OK;
    const size_t bytes = n * msg->point_step;
    HIPCHK(dc->d_raw.ensure(bytes));
    HIPCHK(dc->d_xyz.ensure(n * 16));
    HIPCHK(dc->d_stamp.ensure(n * 8));
    HIPCHK(dc->d_id.ensure(n * 4));
    HIPCHK(hipMemcpyAsync(dc->d_raw.p, msg->data, bytes, hipMemcpyHostToDevice, ctx->stream));
    launch_decode_pointcloud2(dc->d_raw.as<uint8_t>(), (uint32_t)n, msg->point_step, f, sensor, msg->stamp_msg, msg->delta_t_pcs, dc->d_xyz.as<float4>(),
                              dc->d_stamp.as<double>(), dc->d_id.as<int32_t>(), ctx->stream);
    if (field)
        launch_decode_field(dc->d_raw.as<uint8_t>(), (uint32_t)n, msg->point_step, field_offset, field->datatype, dc->d_xyz.as<float>() + 3, 4, ctx->stream);
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}

bool finite_all(const double* v, int k) {
    for (int i = 0; i < k; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

}  // namespace

extern "C" {

void dmsa_default_dense_config(dmsa_dense_config* cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->lidar_to_imu[0] = cfg->lidar_to_imu[5] = cfg->lidar_to_imu[10] = cfg->lidar_to_imu[15] = 1.0f;
}

int dmsa_dense_cloud_create(dmsa_ctx* ctx, const dmsa_dense_config* cfg, const double* stamps, const double* pos, const double* quat_xyzw, int64_t n_p,
                            dmsa_dense_cloud** out) {
    if (out) *out = nullptr;
    if (!ctx || !cfg || !stamps || !pos || !quat_xyzw || !out) return DMSA_ERR_INVALID;
    if (n_p < 2 || n_p > 0x7FFFFFF0) return fail(ctx, DMSA_ERR_INVALID, "dense cloud: a trajectory needs at least two poses");
    if (std::isnan(cfg->min_range) || std::isnan(cfg->max_range) || std::isnan(cfg->voxel_size) || !std::isfinite(cfg->time_offset) ||
        std::isnan(cfg->max_pose_gap) || std::isinf(cfg->voxel_size))
        return fail(ctx, DMSA_ERR_INVALID, "dense cloud: a NaN in the configuration");
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(cfg->lidar_to_imu[i])) return fail(ctx, DMSA_ERR_INVALID, "dense cloud: lidar_to_imu is not finite");
    std::vector<double> q((size_t)n_p * 4);
    for (int64_t k = 0; k < n_p; ++k) {
        if (!std::isfinite(stamps[k]) || (k > 0 && !(stamps[k] > stamps[k - 1])))
            return fail(ctx, DMSA_ERR_INVALID, "dense cloud: stamps must be finite and strictly increasing (pose " + std::to_string(k) + ")");
        if (!finite_all(pos + 3 * k, 3)) return fail(ctx, DMSA_ERR_INVALID, "dense cloud: position of pose " + std::to_string(k) + " is not finite");
        const double* v = quat_xyzw + 4 * k;
        const double nn = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
        if (!finite_all(v, 4) || !(nn > 0.0) || !std::isfinite(nn))
            return fail(ctx, DMSA_ERR_INVALID, "dense cloud: quaternion of pose " + std::to_string(k) + " is zero or not finite");
        q[4 * k] = v[3] / nn, q[4 * k + 1] = v[0] / nn, q[4 * k + 2] = v[1] / nn, q[4 * k + 3] = v[2] / nn;  // (w, x, y, z)
    }
    CHK(set_device(ctx));
    dmsa_dense_cloud* dc = new (std::nothrow) dmsa_dense_cloud();
    if (!dc) return DMSA_ERR_NOMEM;
    dc->ctx = ctx, dc->cfg = *cfg, dc->n_p = n_p;
    DenseGates& g = dc->gates;
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 4; ++col) g.l2i[4 * r + col] = cfg->lidar_to_imu[4 * col + r];
    g.min_range = cfg->min_range, g.max_range = cfg->max_range, g.time_offset = cfg->time_offset, g.max_pose_gap = cfg->max_pose_gap, g.voxel_size = cfg->voxel_size;
    auto build = [&]() -> int {
        HIPCHK(dc->d_stamps.ensure((size_t)n_p * 8));
        HIPCHK(dc->d_pos.ensure((size_t)n_p * 24));
        HIPCHK(dc->d_quat.ensure((size_t)n_p * 32));
        HIPCHK(hipMemcpyAsync(dc->d_stamps.p, stamps, (size_t)n_p * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(dc->d_pos.p, pos, (size_t)n_p * 24, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(dc->d_quat.p, q.data(), (size_t)n_p * 32, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(dc->h_rb.ensure(sizeof(dmsa_dense_cloud::Readback), nullptr));
        HIPCHK(dc->rows.create());
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return DMSA_OK;
    };
    const int rc = build();
    if (rc != DMSA_OK) {
        dmsa_dense_cloud_destroy(dc);
        return rc;
    }
    *out = dc;
    return DMSA_OK;
}

void dmsa_dense_cloud_destroy(dmsa_dense_cloud* dc) {
    if (!dc) return;
    dmsa_ctx* ctx = dc->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamSynchronize(ctx->stream2);
    delete dc;  // (its buffers and events release themselves, an open file is closed; the context's device is current)
}

int dmsa_dense_cloud_interpolate(dmsa_dense_cloud* dc, const double* t, int64_t n, double* pose12_out, int32_t* segment_out) {
    if (!dc || n < 0 || n > kMaxScanPoints || (n > 0 && !t)) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(set_device(ctx));
    if (n == 0 || (!pose12_out && !segment_out)) return DMSA_OK;
    HIPCHK(dc->d_stamp.ensure((size_t)n * 8));
    if (pose12_out) HIPCHK(dc->d_pose12.ensure((size_t)n * 96));
    if (segment_out) HIPCHK(dc->d_seg.ensure((size_t)n * 4));
    HIPCHK(hipMemcpyAsync(dc->d_stamp.p, t, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    launch_dense_interpolate(traj_of(dc), dc->cfg.max_pose_gap, dc->d_stamp.as<double>(), n, pose12_out ? dc->d_pose12.as<double>() : nullptr,
                             segment_out ? dc->d_seg.as<int32_t>() : nullptr, ctx->stream);
    HIPCHK(hipGetLastError());
    if (pose12_out) HIPCHK(hipMemcpyAsync(pose12_out, dc->d_pose12.p, (size_t)n * 96, hipMemcpyDeviceToHost, ctx->stream));
    if (segment_out) HIPCHK(hipMemcpyAsync(segment_out, dc->d_seg.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

int dmsa_dense_cloud_add_scan(dmsa_dense_cloud* dc, const float* xyz, const double* stamps, int64_t n, float* xyz_out, int64_t cap, int64_t* kept,
                              dmsa_dense_stats* call_stats) {
    if (kept) *kept = 0;
    if (!dc || !kept || n < 0 || n > kMaxScanPoints || (n > 0 && (!xyz || !stamps)) || (xyz_out && cap < 0)) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(set_device(ctx));
    if (n > 0) {
        HIPCHK(dc->d_xyz.ensure((size_t)n * 16));
        HIPCHK(dc->d_stamp.ensure((size_t)n * 8));
        HIPCHK(hipMemcpyAsync(dc->d_xyz.p, xyz, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(dc->d_stamp.p, stamps, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    return run_scan(dc, n, xyz_out, cap, kept, call_stats);
}

int dmsa_dense_cloud_add_pointcloud2(dmsa_dense_cloud* dc, const dmsa_pointcloud2* msg, int32_t sensor, float* xyz_out, int64_t cap, int64_t* kept,
                                     dmsa_dense_stats* call_stats) {
    if (kept) *kept = 0;
    if (!dc || !kept || (xyz_out && cap < 0)) return DMSA_ERR_INVALID;
    size_t n = 0;
    CHK(decode_message(dc, msg, sensor, nullptr, &n));
    return run_scan(dc, (int64_t)n, xyz_out, cap, kept, call_stats);
}

// ---- include/dmsa_dense_intensity.h: the switch and the fused path with a field (the headers and the sensors' fields: dense_intensity_text.cpp) ----
int dmsa_dense_cloud_with_intensity(dmsa_dense_cloud* dc) {
    if (!dc) return DMSA_ERR_INVALID;
    if (dc->scan_no != 0 || dc->total.points_in != 0)
        return fail(dc->ctx, DMSA_ERR_INVALID, "dense cloud: with_intensity is legal only before the first scan is added");
    if (dc->file.is_open()) return fail(dc->ctx, DMSA_ERR_INVALID, "dense cloud: with_intensity is legal only before a file is open: " + dc->file.path());
    dc->intensity = true;
    return DMSA_OK;
}

int dmsa_dense_cloud_has_intensity(dmsa_dense_cloud* dc) { return dc ? (dc->intensity ? 1 : 0) : DMSA_ERR_INVALID; }

int dmsa_dense_cloud_add_pointcloud2_field(dmsa_dense_cloud* dc, const dmsa_pointcloud2* msg, int32_t sensor, const dmsa_pointcloud2_field* field, float* xyz_out,
                                           int64_t cap, int64_t* kept, dmsa_dense_stats* call_stats) {
    if (kept) *kept = 0;
    if (!dc || !kept || !field || (xyz_out && cap < 0)) return DMSA_ERR_INVALID;
    if (!dc->intensity) return fail(dc->ctx, DMSA_ERR_INVALID, "dense cloud: the object carries no intensity (dmsa_dense_cloud_with_intensity before the first scan)");
    size_t n = 0;
    CHK(decode_message(dc, msg, sensor, field, &n));
    return run_scan(dc, (int64_t)n, xyz_out, cap, kept, call_stats);
}

int dmsa_dense_cloud_stats(dmsa_dense_cloud* dc, dmsa_dense_stats* total) {
    if (!dc || !total) return DMSA_ERR_INVALID;
    *total = dc->total;
    return DMSA_OK;
}

int dmsa_dense_cloud_reserve(dmsa_dense_cloud* dc, int64_t points) {
    if (!dc || points < 0) return DMSA_ERR_INVALID;
    CHK(set_device(dc->ctx));
    return ensure_table(dc, points);
}

int dmsa_dense_cloud_table_info(dmsa_dense_cloud* dc, int64_t* slots, int64_t* occupied) {
    if (!dc) return DMSA_ERR_INVALID;
    if (slots) *slots = (int64_t)dc->slots;
    if (occupied) *occupied = dc->occupied;
    return DMSA_OK;
}

int dmsa_dense_cloud_open_pcd(dmsa_dense_cloud* dc, const char* path) {
    if (!dc || !path) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    if (dc->file.is_open()) return fail(ctx, DMSA_ERR_INVALID, "dense cloud: a file is open already: " + dc->file.path());
    char header[512];
    const int hn = file_header(dc, 0, header, (int32_t)sizeof(header));
    if (hn < 0) return hn;
    if (!dc->file.open(path, "dense cloud")) return fail(ctx, DMSA_ERR_INVALID, dc->file.why());
    if (!dc->file.write(header, (size_t)hn)) return dc->file.discard(), fail(ctx, DMSA_ERR_INVALID, dc->file.why());
    dc->file_points = 0;
    return DMSA_OK;
}

int dmsa_dense_cloud_close_pcd(dmsa_dense_cloud* dc, int64_t* points, int64_t* bytes) {
    if (points) *points = 0;
    if (bytes) *bytes = 0;
    if (!dc) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    PcdFile& file = dc->file;
    if (!file.is_open()) return fail(ctx, DMSA_ERR_INVALID, "dense cloud: no file is open");
    CHK(set_device(ctx));
    int rc = flush_pending(dc);
    if (rc == DMSA_OK && dc->file_points == 0) rc = fail(ctx, DMSA_ERR_INVALID, "dense cloud: an empty cloud is not written (PCL refuses it): " + file.path() + " removed");
    if (rc == DMSA_OK) {  // WIDTH and POINTS have a fixed width: the header with the counts in it has the length of the one written at open
        char header[512];
        const int hn = file_header(dc, dc->file_points, header, (int32_t)sizeof(header));
        if (hn < 0) rc = hn;
        else if (!file.rewrite_head(header, (size_t)hn) || !file.close()) rc = fail(ctx, DMSA_ERR_INVALID, file.why());
    }
    if (rc != DMSA_OK) return file.discard(), rc;
    if (points) *points = dc->file_points;
    if (bytes) *bytes = file.bytes();
    return DMSA_OK;
}

}  // extern "C"
