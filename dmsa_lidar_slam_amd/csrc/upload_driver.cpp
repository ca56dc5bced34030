// upload_driver.cpp — how a problem becomes resident, for the six upload entries (dmsa_window_upload, dmsa_keyframes_upload: context.cpp;
// dmsa_window_upload_aos, dmsa_keyframes_upload_aos, dmsa_window_upload_from_ring_aos: aos_upload.cpp; dmsa_window_upload_from_ring:
// window_ring.cpp).  An entry checks its arguments and calls upload_window / upload_keyframes with named sources; nothing else uploads.
//
// THE STATE RULE.  An upload is begin -> sources -> commit.
//   * A refusal by an entry's argument checks (null point arrays, negative counts, views, frame offsets, the ring's own refusal) comes before
//     begin and leaves the resident problem exactly as it was.  (The pose arrays are the host model's: for both models begin looks at them.)
//   * upload_begin first WITHDRAWS the resident problem -- model = MODEL_NONE and everything derived from the old points (Gaussians, batch,
//     base table, the voxelisation's guesses) -- then builds the host model, sizes every array of the problem through ensure_problem_buffers
//     and sets the sizes.  upload_commit sets the model as its last statement.  So a failure anywhere between the two (a model the host refuses,
//     an out-of-range tform_idx, an allocation, a HIP error) leaves NO resident problem: every call that needs one returns DMSA_ERR_INVALID.
//   * A later valid upload works as on a fresh context.
// The staging area is used under the one rule of StageArea (dmsa_ctx.h): one acquire per upload, one release behind its last copy; the
// entries that have always ended with a host wait (all but the two ring entries) take StageArea::wait() for it.
#include "dmsa_ctx.h"

namespace {

// what was derived from a problem's points: the current batch and its base table, the Gaussians, the guesses of the next voxelisation
void withdraw_derived_state(dmsa_ctx* ctx) {
    ctx->gaussians_valid = false;
    ctx->batch = 0;
    ctx->base_table = nullptr;
    ctx->vox.forget();
}
void withdraw_resident_problem(dmsa_ctx* ctx) {
    ctx->model = MODEL_NONE;
    ctx->centralized = false;
    withdraw_derived_state(ctx);
}

// [a, b) in one piece, or in one piece per worker thread from 131072 items on (the callers' arrays are pageable: a few threads pack faster)
template <class Fn>
void pack_range(dmsa_ctx* ctx, int64_t a, int64_t b, Fn&& fn) {
    if (b - a < 131072)
        fn(a, b);
    else
        workers(ctx).run_all([&](int t, int nt) { fn(a + (b - a) * t / nt, a + (b - a) * (t + 1) / nt); });
}

// ---- window: the small arrays (all entries), then one source of the moving points and one of the static tail ----
// control stamps, Floater-Hormann weights and the time grid: `area` -> device (the ring's assembly reads the time grid there)
int send_small_arrays(dmsa_ctx* ctx, int64_t n_total, char* area) {
    const size_t C = (size_t)ctx->win.ctrl.n;
    double* sd = reinterpret_cast<double*>(area);
    std::memcpy(sd, ctx->win.stamps.data(), C * 8);
    std::memcpy(sd + C, ctx->win.fh.w.data(), C * 8);
    std::memcpy(sd + 2 * C, ctx->win.traj_time.data(), (size_t)n_total * 8);
    HIPCHK(hipMemcpyAsync(ctx->d_stamps.p, sd, C * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_fhw.p, sd + C, C * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_trajtime.p, sd + 2 * C, (size_t)n_total * 8, hipMemcpyHostToDevice, ctx->stream));
    return DMSA_OK;
}

// Rows [lo, n) packed on the host as the device holds them -- (x, y, z, pose-table row) and the ring id -- then one DMA per array: a window
// point from p's flat arrays (lo = 0), a static point from `st` with the identity row appended to every pose table (lo = N: the tail alone).
int rows_from_host(dmsa_ctx* ctx, const dmsa_window_problem* p, const StaticPoints& st, int64_t lo, char* area) {
    const int64_t N = ctx->N, n = ctx->n;
    if (lo == n) return DMSA_OK;
    float* const loc0 = reinterpret_cast<float*>(area);  // row lo
    int32_t* const ring0 = reinterpret_cast<int32_t*>(area + (size_t)(n - lo) * 16);
    const int32_t id_row = p->n_total;
    std::atomic<bool> bad_row{false};
    pack_range(ctx, lo, n, [&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            float* loc = loc0 + 4 * (i - lo);
            int32_t* ring = ring0 + (i - lo);
            if (i < N) {
                const int32_t row = p->tform_idx[i];
                if (row < 0 || row >= p->n_total) {
                    bad_row = true;
                    return;
                }
                loc[0] = p->xyz_local[4 * i], loc[1] = p->xyz_local[4 * i + 1], loc[2] = p->xyz_local[4 * i + 2];
                std::memcpy(loc + 3, &row, 4);
                *ring = p->ring_id[i];
            } else {
                const size_t k = (size_t)(i - N);
                std::memcpy(loc, st.xyz + k * st.xyz_stride, 12);
                std::memcpy(loc + 3, &id_row, 4);
                std::memcpy(ring, st.id + k * st.id_stride, 4);
            }
        }
    });
    if (bad_row) return fail(ctx, DMSA_ERR_INVALID, "tform_idx out of range");
    HIPCHK(hipMemcpyAsync(ctx->d_local.as<float4>() + lo, loc0, (size_t)(n - lo) * 16, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_ring.as<int32_t>() + lo, ring0, (size_t)(n - lo) * 4, hipMemcpyHostToDevice, ctx->stream));
    return DMSA_OK;
}

// The strided clouds and, riding along, the static tail as raw bytes: [x y z id of every window point | of the static points | tform indices]
// in ONE pass of the worker threads, two DMAs a slice, one pack kernel for the window points and one for the static points.  Of a window point
// only the 16 bytes and its index cross the bus (aos_upload.cpp says why).  The pack kernel checks the rows: this source ends with a host wait.
int raw_from_aos(dmsa_ctx* ctx, const dmsa_window_problem* p, const WindowPoints& pts, const StaticPoints& stat, size_t idx_off, char* st) {
    const int64_t N = ctx->N, S = ctx->S, total = N + S;
    const int num_clouds = pts.num_clouds;
    HIPCHK(ctx->d_aos_raw.ensure(idx_off + 64));
    HIPCHK(ctx->d_aos_idx.ensure((size_t)N * 4 + 64));
    int32_t* d_bad = ctx->d_aos_idx.as<int32_t>() + N;  // one flag word behind the indices
    HIPCHK(hipMemsetAsync(d_bad, 0, 4, ctx->stream));
    std::vector<int64_t> first((size_t)num_clouds + 2, 0);  // prefix of the point counts: clouds, then the static points
    for (int c = 0; c < num_clouds; ++c) first[(size_t)c + 1] = first[(size_t)c] + pts.clouds[c].count;
    first[(size_t)num_clouds + 1] = total;
    auto gather = [&](int64_t a, int64_t b) {  // points [a, b) of the concatenation
        int c = (int)(std::upper_bound(first.begin(), first.end(), a) - first.begin()) - 1;
        for (int64_t i = a; i < b;) {
            while (c <= num_clouds && first[(size_t)c + 1] <= i) ++c;
            const int64_t end = std::min(b, first[(size_t)c + 1]);
            const StaticPoints v = c == num_clouds ? stat : StaticPoints::aos(&pts.clouds[c]);
            for (; i < end; ++i) {
                const size_t k = (size_t)(i - first[(size_t)c]);
                std::memcpy(st + (size_t)i * 16, v.xyz + k * v.xyz_stride, 12);
                std::memcpy(st + (size_t)i * 16 + 12, v.id + k * v.id_stride, 4);
                if (c < num_clouds) std::memcpy(st + idx_off + (size_t)i * 4, pts.clouds[c].index + k, 4);
            }
        }
    };
    // The worker threads gather a slice while the DMA engine moves the slice before it.  (At the bench size the 30 MB over the bus bound the
    // upload either way: 1.8 ms with and without the overlap.)
    const int slices = total < 262144 ? 1 : 8;
    for (int sl = 0; sl < slices; ++sl) {
        const int64_t a = total * sl / slices, b = total * (sl + 1) / slices;
        pack_range(ctx, a, b, gather);
        HIPCHK(hipMemcpyAsync(ctx->d_aos_raw.as<char>() + (size_t)a * 16, st + (size_t)a * 16, (size_t)(b - a) * 16, hipMemcpyHostToDevice, ctx->stream));
        const int64_t ib = std::min(b, N);
        if (a < ib)
            HIPCHK(hipMemcpyAsync(ctx->d_aos_idx.as<char>() + (size_t)a * 4, st + idx_off + (size_t)a * 4, (size_t)(ib - a) * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    ctx->h_stage.release(ctx->stream);
    launch_pack_aos_window(ctx->d_aos_raw.as<uint8_t>(), N, 16, 0, 12, ctx->d_aos_idx.as<int32_t>(), p->n_total, p->n_total, ctx->d_local.as<float4>(),
                           ctx->d_ring.as<int32_t>(), d_bad, ctx->stream);
    launch_pack_aos_window(ctx->d_aos_raw.as<uint8_t>() + (size_t)N * 16, S, 16, 0, 12, nullptr, p->n_total, p->n_total, ctx->d_local.as<float4>() + N,
                           ctx->d_ring.as<int32_t>() + N, d_bad, ctx->stream);
    HIPCHK(hipGetLastError());
    int32_t bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx->h_stage.wait());  // (the entry's one host wait: the verdict and the area)
    return bad ? fail(ctx, DMSA_ERR_INVALID, "tform_idx out of range") : DMSA_OK;
}

// registerPcBuffer (ContinuousTrajectory.h:240-260) on the resident scans, oldest first (RingBuffer::at is chronological)
int points_from_ring(dmsa_ctx* ctx, const dmsa_window_problem* p, double t0) {
    const WindowRing& r = ctx->ring;
    int64_t at = 0;
    for (int k = 0; k < r.filled; ++k) {
        const int slot = (r.head - r.filled + k + 2 * r.num_scans) % r.num_scans;
        const int64_t cnt = r.count[(size_t)slot];
        const size_t off = (size_t)slot * (size_t)r.cap;
        launch_ring_assemble(r.xyz.as<float4>() + off, r.stamp.as<double>() + off, r.id.as<int32_t>() + off, cnt, t0, ctx->d_trajtime.as<double>(), p->n_total,
                             ctx->d_local.as<float4>() + at, ctx->d_ring.as<int32_t>() + at, ctx->stream);
        at += cnt;
    }
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}

int window_sources(dmsa_ctx* ctx, const dmsa_window_problem* p, const WindowPoints& pts, const StaticPoints& st) {
    const size_t N = (size_t)pts.count, S = (size_t)st.count;
    // one area: [stamps | weights | time grid] and behind them what the source stages
    const size_t small = (((size_t)2 * ctx->win.ctrl.n + (size_t)p->n_total) * 8 + 255) & ~(size_t)255;  // (the DMAs of the points start aligned as a device block is)
    const size_t idx_off = ((N + S) * 16 + 15) & ~(size_t)15;  // (AOS) the tform indices behind the raw points
    const size_t part = pts.kind == WindowPoints::FLAT ? (N + S) * 20 : pts.kind == WindowPoints::AOS ? idx_off + N * 4 : S * 20;
    char* area = nullptr;
    HIPCHK(ctx->h_stage.acquire(small + part + 64, &area));
    CHK(send_small_arrays(ctx, p->n_total, area));
    if (pts.kind == WindowPoints::AOS) return raw_from_aos(ctx, p, pts, st, idx_off, area + small);
    CHK(rows_from_host(ctx, p, st, pts.kind == WindowPoints::FLAT ? 0 : ctx->N, area + small));
    ctx->h_stage.release(ctx->stream);
    if (pts.kind == WindowPoints::RING) return points_from_ring(ctx, p, pts.t0);  // (the one source that leaves its work in flight)
    HIPCHK(ctx->h_stage.wait());  // the flat entry has always ended with a host wait
    return DMSA_OK;
}

// ---- keyframes ----
int frames_from_flat(dmsa_ctx* ctx, const dmsa_keyframe_problem* p) {
    const size_t n = (size_t)ctx->n;
    std::vector<float> loc(n * 4);
    for (int k = 0; k < p->num_frames; ++k)
        for (int64_t i = p->frame_offset[k]; i < p->frame_offset[k + 1]; ++i) {
            loc[4 * i] = p->xyz_local[4 * i], loc[4 * i + 1] = p->xyz_local[4 * i + 1], loc[4 * i + 2] = p->xyz_local[4 * i + 2];
            const int32_t row = k;
            std::memcpy(&loc[4 * i + 3], &row, 4);
        }
    HIPCHK(hipMemcpy(ctx->d_local.p, loc.data(), n * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->d_nlocal.p, p->normal_local, n * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->d_ring.p, p->ring_id, n * 4, hipMemcpyHostToDevice));
    return DMSA_OK;
}
// every frame's cloud as it lies in memory, its ring ids as they are; one pack kernel per frame
int frames_from_aos(dmsa_ctx* ctx, const dmsa_keyframe_problem* p, const dmsa_aos_view* frames) {
    size_t raw_bytes = 0;
    for (int k = 0; k < p->num_frames; ++k) raw_bytes += (size_t)frames[k].count * frames[k].stride;
    const size_t idx_off = (raw_bytes + 15) & ~(size_t)15;
    char* st = nullptr;
    HIPCHK(ctx->h_stage.acquire(idx_off + (size_t)ctx->n * 4 + 64, &st));
    HIPCHK(ctx->d_aos_raw.ensure(idx_off + 64));
    size_t at = 0;
    int64_t first = 0;
    for (int k = 0; k < p->num_frames; ++k) {
        const dmsa_aos_view& v = frames[k];
        if (v.count == 0) continue;
        const size_t bytes = (size_t)v.count * v.stride;
        copy_parallel(ctx, st + at, static_cast<const char*>(v.base), bytes);
        HIPCHK(hipMemcpyAsync(ctx->d_aos_raw.as<char>() + at, st + at, bytes, hipMemcpyHostToDevice, ctx->stream));
        std::memcpy(st + idx_off + (size_t)first * 4, v.index, (size_t)v.count * 4);
        HIPCHK(hipMemcpyAsync(ctx->d_ring.as<int32_t>() + first, st + idx_off + (size_t)first * 4, (size_t)v.count * 4, hipMemcpyHostToDevice, ctx->stream));
        launch_pack_aos_keyframe(ctx->d_aos_raw.as<uint8_t>() + at, v.count, v.stride, v.xyz_offset, v.aux_offset, k, ctx->d_local.as<float4>() + first,
                                 ctx->d_nlocal.as<float4>() + first, ctx->stream);
        at += bytes, first += v.count;
    }
    HIPCHK(hipGetLastError());
    ctx->h_stage.release(ctx->stream);
    HIPCHK(ctx->h_stage.wait());  // (as the entry always has)
    return DMSA_OK;
}

// whatever a failed upload enqueued from the staging area has passed before the area is written again
int end_of_upload(dmsa_ctx* ctx, int rc) {
    if (rc != DMSA_OK) ctx->h_stage.release(ctx->stream);
    return rc;
}

}  // namespace

void copy_parallel(dmsa_ctx* ctx, char* dst, const char* src, size_t total) {
    if (total < (size_t)4 << 20) {
        std::memcpy(dst, src, total);
        return;
    }
    workers(ctx).run_all([&](int t, int nt) {
        const size_t a = total * (size_t)t / (size_t)nt, b = total * (size_t)(t + 1) / (size_t)nt;
        std::memcpy(dst + a, src + a, b - a);
    });
}

int ensure_problem_buffers(dmsa_ctx* ctx, int64_t n_points, int rows, bool with_normals) {
    const size_t n = (size_t)n_points;
    const bool keep = ctx->model != MODEL_NONE;  // a reservation beside a resident problem
    auto all = [&]() -> int {
        HIPCHK(ctx->d_local.ensure(n * 16 + 16, keep));
        HIPCHK(ctx->d_ring.ensure(n * 4 + 16, keep));
        if (with_normals) {  // a keyframe problem: normals and no time grid
            HIPCHK(ctx->d_nlocal.ensure(n * 16 + 16, keep));
            HIPCHK(ctx->d_nglobal.ensure(n * 16 + 16, keep));
        } else {  // a window
            HIPCHK(ctx->d_stamps.ensure(64 * 8, keep));  // (at most 64 control poses: upload_begin)
            HIPCHK(ctx->d_fhw.ensure(64 * 8, keep));
            HIPCHK(ctx->d_trajtime.ensure((size_t)(rows - 1) * 8, keep));
        }
        return DMSA_OK;
    };
    const int rc = all();
    if (rc != DMSA_OK && keep) withdraw_resident_problem(ctx);  // an array that could not move is gone
    return rc;
}

int reserve_problem(dmsa_ctx* ctx, int64_t n, int rows, bool with_normals, int P) {
    auto all = [&]() -> int {
        CHK(ensure_problem_buffers(ctx, n, rows, false));
        if (with_normals) CHK(ensure_problem_buffers(ctx, n, rows, true));  // (dmsa_reserve: either model may follow)
        withdraw_derived_state(ctx);  // the buffers below may move; a resident problem's next call derives everything again
        ctx->tablesT_batch = 0, ctx->aabb_fresh = false;
        CHK(alloc_point_buffers(ctx, n));
        HIPCHK(ctx->d_tables.ensure((size_t)(P + 1) * rows * 48));
        HIPCHK(ctx->d_tablesT.ensure((size_t)(P + 1) * rows * 48));
        HIPCHK(ctx->d_table0.ensure((size_t)rows * 48));
        HIPCHK(ctx->d_E.ensure((size_t)(P + 1) * (size_t)(n / 8 + 4096) * 8));  // residual batches: far fewer Gaussians than points in practice (grown on demand otherwise)
        // the loop model holds the addresses of the window's small arrays, which may have moved
        if (ctx->model != MODEL_NONE) CHK(upload_loop_model(ctx, ctx->model));
        return DMSA_OK;
    };
    const int rc = all();
    if (rc != DMSA_OK) withdraw_resident_problem(ctx);  // a buffer that could not grow is empty: nothing resident may go on using it
    return rc;
}

int upload_begin(dmsa_ctx* ctx, const dmsa_window_problem* p, int64_t N, int64_t S) {
    CHK(set_device(ctx));
    withdraw_resident_problem(ctx);
    if (!(p->min_grid_size > 0.0f)) return fail(ctx, DMSA_ERR_INVALID, "invalid window problem (min_grid_size <= 0)");
    if (!ctx->win.init(*p))
        return fail(ctx, DMSA_ERR_INVALID,
                    "invalid window problem (fewer than 3 control poses, coincident stamps, null pose arrays or IMU parameter indices outside the time grid)");
    if (ctx->win.ctrl.n > 64) return fail(ctx, DMSA_ERR_INVALID, "more than 64 control poses");
    CHK(ensure_problem_buffers(ctx, N + S, p->n_total + 1, false));
    ctx->N = N, ctx->S = S, ctx->n = N + S;
    ctx->rows = p->n_total + 1;
    ctx->min_grid_size = p->min_grid_size;
    return DMSA_OK;
}
int upload_begin(dmsa_ctx* ctx, const dmsa_keyframe_problem* p, int64_t n) {
    CHK(set_device(ctx));
    withdraw_resident_problem(ctx);
    if (!p->rel_orient || !p->rel_transl || !(p->min_grid_size > 0.0f)) return fail(ctx, DMSA_ERR_INVALID, "invalid keyframe problem (null pose arrays or min_grid_size <= 0)");
    if (!ctx->key.init(*p)) return DMSA_ERR_INVALID;
    CHK(ensure_problem_buffers(ctx, n, p->num_frames + 1, true));
    ctx->n = n, ctx->N = n, ctx->S = 0;
    ctx->rows = p->num_frames + 1;
    ctx->min_grid_size = p->min_grid_size;
    return DMSA_OK;
}
int upload_commit(dmsa_ctx* ctx, Model model) {
    if (model == MODEL_WINDOW) ctx->win.ctrl.relative_to_global();
    CHK(upload_loop_model(ctx, model));
    CHK(alloc_point_buffers(ctx, ctx->n));
    ctx->model = model;
    return DMSA_OK;
}

int upload_window(dmsa_ctx* ctx, const dmsa_window_problem* p, const WindowPoints& pts, const StaticPoints& st) {
    CHK(upload_begin(ctx, p, pts.count, st.count));
    CHK(end_of_upload(ctx, window_sources(ctx, p, pts, st)));
    return upload_commit(ctx, MODEL_WINDOW);
}
int upload_keyframes(dmsa_ctx* ctx, const dmsa_keyframe_problem* p, int64_t n, const dmsa_aos_view* frames) {
    CHK(upload_begin(ctx, p, n));
    CHK(end_of_upload(ctx, frames ? frames_from_aos(ctx, p, frames) : frames_from_flat(ctx, p)));
    return upload_commit(ctx, MODEL_KEYFRAMES);
}
