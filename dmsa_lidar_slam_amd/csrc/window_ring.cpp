// window_ring.cpp — include/dmsa_window_ring.h: the scans of the sliding window resident in HBM (RingBuffer.h:31-88,
// PointCloudBuffer.h:24-49), one scan uploaded per window, the window problem assembled on the device (ContinuousTrajectory.h:228-261).
#include "dmsa_ctx.h"

#include "../../include/dmsa_window_ring.h"

extern "C" {

int dmsa_window_ring_create(dmsa_ctx* ctx, const dmsa_window_ring_config* cfg) {
    if (!ctx || !cfg || cfg->num_scans < 1 || cfg->num_scans > 1024 || cfg->max_points_per_scan < 1 || cfg->max_static_points < 0 || cfg->max_n_total < 2 ||
        cfg->max_control_poses < 3 || cfg->max_control_poses > 64)
        return DMSA_ERR_INVALID;
    CHK(set_device(ctx));
    WindowRing& r = ctx->ring;
    r.num_scans = cfg->num_scans, r.cap = cfg->max_points_per_scan, r.head = 0, r.filled = 0;
    r.count.assign((size_t)cfg->num_scans, 0);
    const size_t slots = (size_t)cfg->num_scans * (size_t)cfg->max_points_per_scan;
    HIPCHK(r.xyz.ensure(slots * 16));
    HIPCHK(r.stamp.ensure(slots * 8));
    HIPCHK(r.id.ensure(slots * 4));
    // one pinned staging area for a scan (28 bytes per point) or the static points of a window (20 bytes per point)
    const size_t stage = std::max((size_t)cfg->max_points_per_scan * 28, (size_t)cfg->max_static_points * 20) + 256;
    HIPCHK(ctx->h_stage.acquire(stage));
    // every buffer whose size depends on the point count, for the full window: nothing is allocated when the windows start to slide
    CHK(reserve_problem(ctx, (int64_t)slots + cfg->max_static_points, cfg->max_n_total + 1, false, 6 * (cfg->max_control_poses - 1)));
    return DMSA_OK;
}

int dmsa_window_ring_push(dmsa_ctx* ctx, const float* xyz_local, const double* stamps, const int32_t* ring_id, int64_t n) {
    if (!ctx || ctx->ring.num_scans == 0 || n < 0 || n > ctx->ring.cap || (n > 0 && (!xyz_local || !stamps || !ring_id))) return DMSA_ERR_INVALID;
    CHK(set_device(ctx));
    WindowRing& r = ctx->ring;
    const int slot = r.head;
    // RingBuffer::addElem (RingBuffer.h:67-88): the oldest element is overwritten once the buffer is full
    const size_t off = (size_t)slot * (size_t)r.cap;
    if (n > 0) {
        char* st = nullptr;
        HIPCHK(ctx->h_stage.acquire((size_t)n * 28, &st));
        std::memcpy(st, xyz_local, (size_t)n * 16);
        std::memcpy(st + (size_t)n * 16, stamps, (size_t)n * 8);
        std::memcpy(st + (size_t)n * 24, ring_id, (size_t)n * 4);
        HIPCHK(hipMemcpyAsync(r.xyz.as<char>() + off * 16, st, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(r.stamp.as<char>() + off * 8, st + (size_t)n * 16, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(r.id.as<char>() + off * 4, st + (size_t)n * 24, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        ctx->h_stage.release(ctx->stream);
    }
    r.count[(size_t)slot] = n;
    r.head = (r.head + 1) % r.num_scans;
    r.filled = std::min(r.filled + 1, r.num_scans);
    return DMSA_OK;
}

int dmsa_window_ring_points(dmsa_ctx* ctx, int32_t* scans_out, int64_t* points_out) {
    if (!ctx || ctx->ring.num_scans == 0) return DMSA_ERR_INVALID;
    int64_t total = 0;
    for (int k = 0; k < ctx->ring.filled; ++k) total += ctx->ring.count[(size_t)((ctx->ring.head - ctx->ring.filled + k + 2 * ctx->ring.num_scans) % ctx->ring.num_scans)];
    if (scans_out) *scans_out = ctx->ring.filled;
    if (points_out) *points_out = total;
    return DMSA_OK;
}

}  // extern "C"

int ring_upload_checks(dmsa_ctx* ctx, float min_grid_size, int64_t num_points, bool static_arrays_ok, int64_t* N) {
    if (ctx->ring.num_scans == 0) return DMSA_ERR_INVALID;
    CHK(dmsa_window_ring_points(ctx, nullptr, N));
    if ((num_points != 0 && num_points != *N) || !static_arrays_ok || !(min_grid_size > 0.0f))
        return fail(ctx, DMSA_ERR_INVALID,
                    "invalid window problem for the resident ring (point count differs from the ring's, null static arrays or min_grid_size <= 0)");
    return DMSA_OK;
}

extern "C" {

int dmsa_window_upload_from_ring(dmsa_ctx* ctx, const dmsa_window_problem* p, double t0) {
    if (!ctx || !p || p->num_static < 0) return DMSA_ERR_INVALID;
    int64_t N = 0;
    CHK(ring_upload_checks(ctx, p->min_grid_size, p->num_points, p->num_static == 0 || (p->xyz_static && p->ring_id_static), &N));
    return upload_window(ctx, p, WindowPoints::ring(N, t0), StaticPoints::flat(p));
}

}  // extern "C"
