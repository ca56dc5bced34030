// dense_normals_api.cpp — include/dmsa_dense_normals.h on top of dense_normals.hip: the retained store of a dense cloud object (N0), the search
// grid over it (cell keys, the library's stable 64-bit sort, the cell table), the launch sequence of the moments and the normals, and the
// binary PCD files of the store (chunks through copy_back.h into a pcd_file.h).  The header text and N4 on the host: dense_normals_text.cpp.
// The state, the grid, N1's checks of the radius and the file writer are shared with dense_outliers_api.cpp (dense_cloud_obj.h).
#include "dense_cloud_obj.h"

#include "dense_normals.h"

void dense_normals_release(dmsa_dense_cloud* dc) {
    delete dc->nrm;  // (its buffers and events release themselves)
    dc->nrm = nullptr;
}

void dense_normals_invalidate(dmsa_dense_cloud* dc) {
    if (dc->nrm) dc->nrm->grid_n = 0, dc->nrm->normals_valid = false, dc->nrm->flags_n = -1, dc->nrm->carve_n = -1;
}

namespace {

constexpr int64_t kMaxRetained = 0x7FFFFFF0;       // a sorted row index fits the uint32 of the sort's values
constexpr int64_t kFileChunkRows = (int64_t)1 << 20;  // 28 MiB per pinned buffer

// N1
int check_preconditions(dmsa_dense_cloud* dc, const dmsa_dense_normals_config* cfg) {
    CHK(dense_radius_preconditions(dc, cfg->radius, "dense normals"));
    if (cfg->min_neighbours < 0) return fail(dc->ctx, DMSA_ERR_INVALID, "dense normals: min_neighbours must be >= 0");
    return DMSA_OK;
}

// N2-N3 for rows [first, first + count) into st->moments
int run_moments(dmsa_dense_cloud* dc, DenseNormalsState* st, const dmsa_dense_normals_config* cfg, int64_t first, int64_t count) {
    dmsa_ctx* ctx = dc->ctx;
    CHK(dense_normals_grid(dc, st, dense_radius_edge(cfg->radius)));
    HIPCHK(st->moments.ensure((size_t)count * 80));
    int e = 0;
    (void)std::frexp(cfg->radius, &e);
    const float scale = std::ldexp(1.0f, 20 - e), r2 = cfg->radius * cfg->radius;
    launch_neighbour_moments(st->pts.as<float4>(), st->idx_s.as<uint32_t>(), st->key_s.as<unsigned long long>(), dc->ret_n, st->table.as<DenseCellEntry>(), st->mask, r2,
                             scale, first, count, st->moments.as<long long>(), ctx->stream);
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}

// header + rows of `row_floats` floats (7: x y z and the normal, 3: x y z), a chunk of kFileChunkRows rows at a time
int write_rows(dmsa_dense_cloud* dc, DenseNormalsState* st, PcdFile& file, int row_floats) {
    dmsa_ctx* ctx = dc->ctx;
    const int64_t n = dc->ret_n;
    const size_t row_bytes = (size_t)row_floats * 4;
    char header[512];
    const int hn = row_floats == 7 ? dmsa_pcd_header_normals_binary(n, header, (int32_t)sizeof(header)) : dmsa_pcd_header_xyz_binary(n, header, (int32_t)sizeof(header));
    if (hn < 0) return hn;
    if (!file.write(header, (size_t)hn)) return fail(ctx, DMSA_ERR_INVALID, file.why());
    const int64_t chunk = std::min(kFileChunkRows, n);
    auto rows_of = [&](int64_t c) { return std::min(chunk, n - c * chunk); };
    for (int b = 0; b < 2; ++b) HIPCHK(st->rows.reserve(b, (size_t)chunk * row_bytes, (size_t)chunk * row_bytes));
    auto pack = [&](int64_t c, int b) -> int {
        float* out = st->rows.dev[b].as<float>();
        if (row_floats == 7) launch_pack_normal_rows(dc->ret_g.as<float4>(), st->normal.as<float4>(), c * chunk, rows_of(c), out, ctx->stream);
        else launch_dense_pack_rows(dc->ret_g.as<float4>() + c * chunk, rows_of(c), out, ctx->stream);
        HIPCHK(hipGetLastError());
        return DMSA_OK;
    };
    auto bytes_of = [&](int64_t c, int, size_t* bytes) -> int { return *bytes = (size_t)rows_of(c) * row_bytes, DMSA_OK; };
    return copy_back_chunks(ctx, st->rows, file, (n + chunk - 1) / chunk, pack, bytes_of);
}

}  // namespace

int dense_normals_state(dmsa_dense_cloud* dc, DenseNormalsState** out) {
    dmsa_ctx* ctx = dc->ctx;
    if (!dc->nrm) {
        DenseNormalsState* st = new (std::nothrow) DenseNormalsState();
        if (!st) return DMSA_ERR_NOMEM;
        dc->nrm = st;
        HIPCHK(st->h_counter.ensure(2 * sizeof(unsigned long long), nullptr));
        HIPCHK(st->counter.ensure(2 * sizeof(unsigned long long)));
        HIPCHK(st->rows.create());
    }
    *out = dc->nrm;
    return DMSA_OK;
}

// what N1 asks of the store and of `radius` (`what` opens the reason: "dense normals" or "dense outliers")
int dense_radius_preconditions(dmsa_dense_cloud* dc, float r, const char* what) {
    dmsa_ctx* ctx = dc->ctx;
    const std::string w = std::string(what) + ": ";
    if (!dc->retain) return fail(ctx, DMSA_ERR_INVALID, w + "retention is off (dmsa_dense_cloud_retain before the first scan)");
    if (dc->ret_n < 1) return fail(ctx, DMSA_ERR_INVALID, w + "no retained point");
    const float v = dc->cfg.voxel_size;
    if (!(v > 0.0f)) return fail(ctx, DMSA_ERR_INVALID, w + "voxel_size must be > 0");
    if (!std::isfinite(r)) return fail(ctx, DMSA_ERR_INVALID, w + "radius is not finite");
    if (!(r >= v && r <= 64.0f * v)) return fail(ctx, DMSA_ERR_INVALID, w + "radius must lie in [voxel_size, 64 * voxel_size]");
    int e = 0;
    (void)std::frexp(r, &e);
    if (20 - e > 126) return fail(ctx, DMSA_ERR_INVALID, w + "radius is too small for the scale of N3");
    return DMSA_OK;
}

// the search grid over all retained rows with cells of this edge (kept until a scan is added or the edge changes)
int dense_normals_grid(dmsa_dense_cloud* dc, DenseNormalsState* st, double edge) {
    dmsa_ctx* ctx = dc->ctx;
    const int64_t n = dc->ret_n;
    if (st->grid_n == n && st->grid_edge == edge) return DMSA_OK;
    st->grid_n = 0;
    const size_t un = (size_t)n;
    HIPCHK(st->key.ensure(un * 8));
    HIPCHK(st->key_s.ensure(un * 8));
    HIPCHK(st->idx.ensure(un * 4));
    HIPCHK(st->idx_s.ensure(un * 4));
    HIPCHK(st->pts.ensure(un * 16));
    HIPCHK(st->sort_tmp.ensure(sort_pairs_temp_bytes(un)));
    launch_normals_cell_keys(dc->ret_g.as<float4>(), n, edge, st->key.as<unsigned long long>(), st->idx.as<uint32_t>(), ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(sort_pairs_u64_u32(st->sort_tmp.p, st->sort_tmp.cap, st->key.as<uint64_t>(), st->key_s.as<uint64_t>(), st->idx.as<uint32_t>(), st->idx_s.as<uint32_t>(), un, 63,
                              0, ctx->stream));
    unsigned long long* counter = st->counter.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(counter, 0, 16, ctx->stream));
    launch_normals_count_cells(st->key_s.as<unsigned long long>(), n, counter, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(st->h_counter.p, counter, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const uint64_t cells = st->h_counter.as<unsigned long long>()[0];
    uint64_t slots = 1024;
    while (slots < 2 * cells) slots <<= 1;  // never more than half full; cells <= n < 2^31
    HIPCHK(st->table.ensure((size_t)slots * sizeof(DenseCellEntry)));
    HIPCHK(hipMemsetAsync(st->table.p, 0xFF, (size_t)slots * sizeof(DenseCellEntry), ctx->stream));
    st->mask = (uint32_t)(slots - 1);
    launch_normals_cell_heads(dc->ret_g.as<float4>(), st->idx_s.as<uint32_t>(), st->key_s.as<unsigned long long>(), n, st->pts.as<float4>(),
                              st->table.as<DenseCellEntry>(), st->mask, ctx->stream);
    launch_normals_cell_ends(st->key_s.as<unsigned long long>(), n, st->table.as<DenseCellEntry>(), st->mask, ctx->stream);
    HIPCHK(hipGetLastError());
    st->grid_n = n, st->grid_edge = edge;
    return DMSA_OK;
}

int dense_compact_store(dmsa_dense_cloud* dc, const int32_t* keep, const int32_t* keep_scan, int64_t m, const char* what) {
    dmsa_ctx* ctx = dc->ctx;
    const int64_t n = dc->ret_n, cap = std::max<int64_t>(m, 1);
    DevBuf g, o;
    if (g.ensure((size_t)cap * 16) != hipSuccess || o.ensure((size_t)cap * 16) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, DMSA_ERR_NOMEM, std::string(what) + ": no device memory for a retained store of " + std::to_string(cap) + " points");
    }
    launch_dense_scatter(dc->ret_g.as<float4>(), keep, keep_scan, n, g.as<float4>(), ctx->stream);
    launch_dense_scatter(dc->ret_o.as<float4>(), keep, keep_scan, n, o.as<float4>(), ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    dc->ret_g.swap(g), dc->ret_o.swap(o);
    dc->ret_n = m, dc->ret_cap = cap;
    dense_normals_invalidate(dc);  // classifications, grid and normals were of the store before
    return DMSA_OK;                // (`g` and `o` free the old store)
}

int dense_save_rows(dmsa_dense_cloud* dc, DenseNormalsState* st, const char* path, const char* what, int row_floats, int64_t* points_out, int64_t* bytes_out) {
    dmsa_ctx* ctx = dc->ctx;
    CHK(set_device(ctx));
    PcdFile file;
    if (!file.open(path, what)) return fail(ctx, DMSA_ERR_INVALID, file.why());
    const int rc = copy_back_end(ctx, file, write_rows(dc, st, file, row_floats));
    if (rc != DMSA_OK) return file.discard(), rc;
    if (points_out) *points_out = dc->ret_n;
    if (bytes_out) *bytes_out = file.bytes();
    return DMSA_OK;
}

int dense_retain_reserve(dmsa_dense_cloud* dc, int64_t m) {
    dmsa_ctx* ctx = dc->ctx;
    const int64_t need = dc->ret_n + m;
    if (need <= dc->ret_cap) return DMSA_OK;
    if (need > kMaxRetained) return fail(ctx, DMSA_ERR_NOMEM, "dense cloud: the retained store would exceed 2^31 points");
    int64_t cap = std::max<int64_t>(dc->ret_cap, 4096);
    while (cap < need) cap *= 2;
    cap = std::min(cap, kMaxRetained);
    DevBuf g, o;
    if (g.ensure((size_t)cap * 16) != hipSuccess || o.ensure((size_t)cap * 16) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, DMSA_ERR_NOMEM, "dense cloud: no device memory for a retained store of " + std::to_string(cap) + " points");
    }
    if (dc->ret_n > 0) {
        HIPCHK(hipMemcpyAsync(g.p, dc->ret_g.p, (size_t)dc->ret_n * 16, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(o.p, dc->ret_o.p, (size_t)dc->ret_n * 16, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    dc->ret_g.swap(g), dc->ret_o.swap(o);
    dc->ret_cap = cap;
    return DMSA_OK;  // (`g` and `o` free the old store)
}

int dense_retain_append(dmsa_dense_cloud* dc, int64_t m) {
    dmsa_ctx* ctx = dc->ctx;
    if (dc->ret_n + m > dc->ret_cap) return DMSA_ERR_INVALID;  // (never: dense_retain_reserve ran)
    HIPCHK(hipMemcpyAsync(dc->ret_g.as<float4>() + dc->ret_n, dc->d_out.p, (size_t)m * 16, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(dc->ret_o.as<float4>() + dc->ret_n, dc->d_out_o.p, (size_t)m * 16, hipMemcpyDeviceToDevice, ctx->stream));
    return DMSA_OK;
}

extern "C" {

int dmsa_dense_cloud_retain(dmsa_dense_cloud* dc) {
    if (!dc) return DMSA_ERR_INVALID;
    if (dc->scan_no != 0 || dc->total.points_in != 0) return fail(dc->ctx, DMSA_ERR_INVALID, "dense cloud: retain is legal only before the first scan is added");
    dc->retain = true;
    return DMSA_OK;
}

int dmsa_dense_cloud_retained(dmsa_dense_cloud* dc, int64_t first, int64_t count, float* xyz_out, float* origin_out, int64_t* total_out) {
    if (total_out) *total_out = 0;
    if (!dc || first < 0 || count < 0) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    if (!dc->retain) return fail(ctx, DMSA_ERR_INVALID, "dense cloud: retention is off (dmsa_dense_cloud_retain before the first scan)");
    if (total_out) *total_out = dc->ret_n;
    if (first > dc->ret_n || count > dc->ret_n - first) return fail(ctx, DMSA_ERR_INVALID, "dense cloud: rows beyond the retained store");
    CHK(set_device(ctx));
    if (count == 0) return DMSA_OK;
    if (xyz_out) HIPCHK(hipMemcpyAsync(xyz_out, dc->ret_g.as<float4>() + first, (size_t)count * 16, hipMemcpyDeviceToHost, ctx->stream));
    if (origin_out) HIPCHK(hipMemcpyAsync(origin_out, dc->ret_o.as<float4>() + first, (size_t)count * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

int dmsa_dense_cloud_neighbour_moments(dmsa_dense_cloud* dc, const dmsa_dense_normals_config* cfg, int64_t first, int64_t count, int64_t* moments) {
    if (!dc || !cfg || first < 0 || count < 0 || (count > 0 && !moments)) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    if (first > dc->ret_n || count > dc->ret_n - first) return fail(ctx, DMSA_ERR_INVALID, "dense normals: rows beyond the retained store");
    if (count == 0) return DMSA_OK;
    CHK(set_device(ctx));
    DenseNormalsState* st = nullptr;
    CHK(dense_normals_state(dc, &st));
    CHK(run_moments(dc, st, cfg, first, count));
    HIPCHK(hipMemcpyAsync(moments, st->moments.p, (size_t)count * 80, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

int dmsa_dense_cloud_compute_normals(dmsa_dense_cloud* dc, const dmsa_dense_normals_config* cfg, float* normal_out, int64_t* total, int64_t* without_normal) {
    if (total) *total = 0;
    if (without_normal) *without_normal = 0;
    if (!dc || !cfg) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(set_device(ctx));
    DenseNormalsState* st = nullptr;
    CHK(dense_normals_state(dc, &st));
    st->normals_valid = false;
    const int64_t n = dc->ret_n;
    CHK(run_moments(dc, st, cfg, 0, n));
    HIPCHK(st->normal.ensure((size_t)n * 16));
    unsigned long long* without = st->counter.as<unsigned long long>() + 1;
    HIPCHK(hipMemsetAsync(without, 0, 8, ctx->stream));
    launch_normals_from_moments(st->moments.as<long long>(), dc->ret_g.as<float4>(), dc->ret_o.as<float4>(), 0, n, cfg->min_neighbours, st->normal.as<float4>(),
                                without, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(st->h_counter.as<unsigned long long>() + 1, without, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (normal_out) HIPCHK(hipMemcpyAsync(normal_out, st->normal.p, (size_t)n * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    st->moments.release();  // 80 bytes per row: not kept beside the result
    st->normals_valid = true;
    if (total) *total = n;
    if (without_normal) *without_normal = (int64_t)st->h_counter.as<unsigned long long>()[1];
    return DMSA_OK;
}

int dmsa_dense_cloud_save_pcd_normals(dmsa_dense_cloud* dc, const char* path, int64_t* points_out, int64_t* bytes_out) {
    if (points_out) *points_out = 0;
    if (bytes_out) *bytes_out = 0;
    if (!dc || !path) return DMSA_ERR_INVALID;
    DenseNormalsState* st = dc->nrm;
    if (!st || !st->normals_valid || dc->ret_n < 1)
        return fail(dc->ctx, DMSA_ERR_INVALID, "dense normals: no normals since the last added scan (dmsa_dense_cloud_compute_normals first)");
    return dense_save_rows(dc, st, path, "dense normals", 7, points_out, bytes_out);
}

}  // extern "C"
