// aos_upload.cpp — include/dmsa_aos.h: the reference's point containers (pcl::PointCloud<PointStampId>, 32-byte points,
// PointStampId.h:33-45; pcl::PointCloud<pcl::PointNormal>, 48-byte points, KeyframeData.h:20) handed over as they lie in memory.
// Here: the entries' argument checks; the uploads themselves are upload_driver.cpp's.  Host side: the worker threads move what the device
// needs into pinned staging -- of a window point the 16 bytes x, y, z, id plus its tform index, so that a scan crosses PCIe as 20 bytes per
// point like the flat arrays (measured: the whole 32-byte points cost 0.7 ms more per call than the gather saves) -- and the pack kernels
// (static_kernels.hip) write the layouts of dmsa_ctx.h.
#include "dmsa_ctx.h"

#include "../../include/dmsa_window_ring.h"

namespace {

bool view_ok(const dmsa_aos_view& v, int min_aux_bytes) {
    if (v.count < 0 || (v.count > 0 && !v.base)) return false;
    if (v.stride < 16 || (v.stride & 3) != 0 || v.xyz_offset < 0 || (v.xyz_offset & 3) != 0 || v.xyz_offset + 12 > v.stride) return false;
    return v.aux_offset >= 0 && (v.aux_offset & 3) == 0 && v.aux_offset + min_aux_bytes <= v.stride;
}

}  // namespace

extern "C" {

int dmsa_window_upload_aos(dmsa_ctx* ctx, const dmsa_window_problem* p, const dmsa_aos_view* clouds, int32_t num_clouds, const dmsa_aos_view* static_points) {
    if (!ctx || !p || num_clouds < 0 || (num_clouds > 0 && !clouds)) return DMSA_ERR_INVALID;
    int64_t N = 0;
    for (int c = 0; c < num_clouds; ++c) {
        if (!view_ok(clouds[c], 4) || (clouds[c].count > 0 && !clouds[c].index)) {
            ctx->err = "invalid window cloud view (stride / offsets not multiples of four, fields outside the point, or no tform indices)";
            return DMSA_ERR_INVALID;
        }
        N += clouds[c].count;
    }
    const int64_t S = static_points ? static_points->count : 0;
    if (S < 0 || (S > 0 && !view_ok(*static_points, 4))) {
        ctx->err = "invalid static point view";
        return DMSA_ERR_INVALID;
    }
    return upload_window(ctx, p, WindowPoints::aos(clouds, num_clouds, N), StaticPoints::aos(S > 0 ? static_points : nullptr));
}

int dmsa_keyframes_upload_aos(dmsa_ctx* ctx, const dmsa_keyframe_problem* p, const dmsa_aos_view* frames, int32_t num_frames) {
    if (!ctx || !p || !frames || num_frames != p->num_frames || num_frames < 2) return DMSA_ERR_INVALID;
    int64_t n = 0;
    for (int k = 0; k < num_frames; ++k) {
        if (!view_ok(frames[k], 16) || (frames[k].count > 0 && !frames[k].index)) {
            ctx->err = "invalid keyframe cloud view (stride / offsets not multiples of four, fields outside the point, or no ring ids)";
            return DMSA_ERR_INVALID;
        }
        n += frames[k].count;
    }
    return upload_keyframes(ctx, p, n, frames);
}

int dmsa_optimize_window_aos(dmsa_ctx* ctx, dmsa_window_problem* p, const dmsa_aos_view* clouds, int32_t num_clouds, const dmsa_aos_view* static_points,
                             const dmsa_settings* s, dmsa_report* rep) {
    if (!ctx || !p || !s) return DMSA_ERR_INVALID;
    CHK(dmsa_window_upload_aos(ctx, p, clouds, num_clouds, static_points));
    CHK(optimize(ctx, *s, rep));
    write_back_poses(ctx->win.ctrl, p->rel_orient, p->rel_transl);
    return DMSA_OK;
}

int dmsa_optimize_keyframes_aos(dmsa_ctx* ctx, dmsa_keyframe_problem* p, const dmsa_aos_view* frames, int32_t num_frames, const dmsa_settings* s, dmsa_report* rep) {
    if (!ctx || !p || !s) return DMSA_ERR_INVALID;
    CHK(dmsa_keyframes_upload_aos(ctx, p, frames, num_frames));
    CHK(optimize(ctx, *s, rep));
    write_back_poses(ctx->key.frames, p->rel_orient, p->rel_transl);
    return DMSA_OK;
}

int dmsa_get_global_points_aos(dmsa_ctx* ctx, void* base, int64_t count, int32_t stride, int32_t xyz_offset, int32_t normal_offset) {
    if (!ctx || ctx->model == MODEL_NONE || !base || count < ctx->n || stride < 16 || (stride & 3) || xyz_offset < 0 || xyz_offset + 12 > stride ||
        (normal_offset >= 0 && (normal_offset + 12 > stride || ctx->model != MODEL_KEYFRAMES)))
        return DMSA_ERR_INVALID;
    CHK(set_device(ctx));
    const size_t n = (size_t)ctx->n, per = normal_offset >= 0 ? 32 : 16;
    char* area = nullptr;
    HIPCHK(ctx->h_stage.acquire(n * per + 64, &area));
    float* xyz = reinterpret_cast<float*>(area);
    float* nrm = xyz + 4 * n;
    // Pieces of <= 2^18 points come down one after the other; the worker threads scatter a piece into the caller's container while the
    // DMA engine fetches the next ones.
    struct Piece {
        size_t first, count;   // points
        const float* src;      // staging
        int field;             // byte offset of the three floats inside a point of the container
        hipEvent_t done;
    };
    std::vector<Piece> pieces;
    auto fetch = [&](float* dst, const void* dev, size_t first, size_t count, int field) -> int {
        constexpr size_t kPiece = (size_t)1 << 18;
        for (size_t a = 0; a < count; a += kPiece) {
            const size_t c = std::min(kPiece, count - a);
            HIPCHK(hipMemcpyAsync(dst + 4 * (first + a), static_cast<const char*>(dev) + a * 16, c * 16, hipMemcpyDeviceToHost, ctx->stream));
            Piece pc{first + a, c, dst, field, nullptr};
            HIPCHK(hipEventCreateWithFlags(&pc.done, hipEventDisableTiming));
            pieces.push_back(pc);
            HIPCHK(hipEventRecord(pc.done, ctx->stream));
        }
        return DMSA_OK;
    };
    int rc = fetch(xyz, ctx->d_global.p, 0, (size_t)ctx->N, xyz_offset);
    if (rc == DMSA_OK && ctx->model == MODEL_WINDOW && ctx->S > 0)  // static points are not moved by updateGlobalPoints; they sit (de-centralised again) in the local array
        rc = fetch(xyz, ctx->d_local.as<float4>() + ctx->N, (size_t)ctx->N, (size_t)ctx->S, xyz_offset);
    if (rc == DMSA_OK && normal_offset >= 0) rc = fetch(nrm, ctx->d_nglobal.p, 0, n, normal_offset);
    char* out = static_cast<char*>(base);
    for (Piece& pc : pieces) {
        if (rc == DMSA_OK && hipEventSynchronize(pc.done) != hipSuccess) ctx->err = "hipEventSynchronize failed", rc = DMSA_ERR_HIP;
        if (rc == DMSA_OK) {
            auto scatter = [&](size_t a, size_t b) {
                for (size_t i = a; i < b; ++i) std::memcpy(out + i * (size_t)stride + pc.field, pc.src + 4 * i, 12);
            };
            if (pc.count < 65536)
                scatter(pc.first, pc.first + pc.count);
            else
                workers(ctx).run_all([&](int t, int nt) {
                    scatter(pc.first + pc.count * (size_t)t / (size_t)nt, pc.first + pc.count * (size_t)(t + 1) / (size_t)nt);
                });
        }
        (void)hipEventDestroy(pc.done);
    }
    if (rc != DMSA_OK) ctx->h_stage.release(ctx->stream);  // (a call that succeeded has waited for every piece)
    return rc;
}

int dmsa_window_ring_push_aos(dmsa_ctx* ctx, const dmsa_aos_view* scan, int32_t stamp_offset) {
    if (!ctx || !scan || ctx->ring.num_scans == 0 || !view_ok(*scan, 4) || scan->count > ctx->ring.cap || stamp_offset < 0 || (stamp_offset & 3) != 0 ||
        stamp_offset + 8 > scan->stride)
        return DMSA_ERR_INVALID;
    CHK(set_device(ctx));
    WindowRing& r = ctx->ring;
    const int slot = r.head;  // RingBuffer::addElem (RingBuffer.h:67-88): the oldest element is overwritten once the buffer is full
    const size_t off = (size_t)slot * (size_t)r.cap, bytes = (size_t)scan->count * scan->stride;
    if (scan->count > 0) {
        char* area = nullptr;
        HIPCHK(ctx->h_stage.acquire(bytes + 64, &area));
        HIPCHK(ctx->d_aos_raw.ensure(bytes + 64));
        copy_parallel(ctx, area, static_cast<const char*>(scan->base), bytes);
        HIPCHK(hipMemcpyAsync(ctx->d_aos_raw.p, area, bytes, hipMemcpyHostToDevice, ctx->stream));
        ctx->h_stage.release(ctx->stream);
        launch_unpack_ring_scan(ctx->d_aos_raw.as<uint8_t>(), scan->count, scan->stride, scan->xyz_offset, stamp_offset, scan->aux_offset, r.xyz.as<float4>() + off,
                                r.stamp.as<double>() + off, r.id.as<int32_t>() + off, ctx->stream);
        HIPCHK(hipGetLastError());
    }
    r.count[(size_t)slot] = scan->count;
    r.head = (r.head + 1) % r.num_scans;
    r.filled = std::min(r.filled + 1, r.num_scans);
    return DMSA_OK;
}

int dmsa_window_upload_from_ring_aos(dmsa_ctx* ctx, const dmsa_window_problem* p, double t0, const dmsa_aos_view* static_points) {
    if (!ctx || !p) return DMSA_ERR_INVALID;
    const int64_t S = static_points ? static_points->count : 0;
    if (S < 0 || (S > 0 && !view_ok(*static_points, 4))) return DMSA_ERR_INVALID;
    // the window points come from the ring (p's point arrays are ignored), the static tail of globalPoints from its container
    int64_t N = 0;
    CHK(ring_upload_checks(ctx, p->min_grid_size, 0, true, &N));
    return upload_window(ctx, p, WindowPoints::ring(N, t0), StaticPoints::aos(S > 0 ? static_points : nullptr));
}

int dmsa_reserve(dmsa_ctx* ctx, int64_t max_points, int32_t max_table_rows, int32_t max_params) {
    if (!ctx || max_points < 1 || max_table_rows < 1 || max_params < 6) return DMSA_ERR_INVALID;
    CHK(set_device(ctx));
    const size_t n = (size_t)max_points;
    HIPCHK(ctx->d_aos_raw.ensure(n * 48 + 64));
    HIPCHK(ctx->d_aos_idx.ensure(n * 4 + 64));
    HIPCHK(ctx->d_static_keep.ensure(n * 16));
    HIPCHK(ctx->h_stage.acquire(n * 52 + 128));
    CHK(reserve_problem(ctx, max_points, max_table_rows + 1, true, max_params));
    return DMSA_OK;
}

}  // extern "C"
