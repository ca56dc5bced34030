// dense_store.cpp — what the stages over the dense cloud stand on (dense_cloud_obj.h): the retained store of a dense cloud object (N0), the
// search grid over it (cell keys, the library's stable 64-bit sort, the cell table: dense_grid.hip), a row mask and the removal by one, the
// preconditions every stage asks, and the binary PCD files of the store (chunks through copy_back.h into a pcd_file.h).
#include "dense_cloud_obj.h"

#include "dense_compare.h"
#include "dense_normals.h"

namespace {

constexpr int64_t kMaxRetained = 0x7FFFFFF0;          // a sorted row index fits the uint32 of the sort's values
constexpr int64_t kMaxStageRows = (int64_t)1 << 26;   // O1, T1
constexpr int64_t kFileChunkRows = (int64_t)1 << 20;  // at most 32 MiB per pinned buffer

// header + rows of `row_floats` floats (3: x y z, 7: x y z and the normal; 4 and 8: the same with the intensity after z) and, with `word`,
// the row's cluster label or its distance to the reference behind them, a chunk of kFileChunkRows rows at a time
int write_rows(dmsa_dense_cloud* dc, PcdFile& file, int row_floats, RowWord word) {
    dmsa_ctx* ctx = dc->ctx;
    CopyBack& back = dc->shared.files;
    const int64_t n = dc->store.n;
    const bool labels = word == RowWord::label, distance = word == RowWord::distance, extra = labels || distance;
    if (extra && row_floats > 4) return DMSA_ERR_INVALID;  // (never: C7 and D7 have no normals)
    // the extra word's buffer: the packing kernel copies 32 bits per row, a label's or a float's alike
    const int32_t* words = labels ? dc->clusters.label.as<int32_t>() : distance ? dc->compare.dist[0].as<int32_t>() : nullptr;
    const size_t row_bytes = (size_t)(row_floats + (extra ? 1 : 0)) * 4;
    char header[512];
    const int32_t hcap = (int32_t)sizeof(header);
    const int hn = labels            ? dmsa_pcd_header_xyz_label_binary(n, row_floats == 4, header, hcap)
                   : distance        ? dmsa_pcd_header_xyz_distance_binary(n, row_floats == 4, header, hcap)
                   : row_floats == 8 ? dmsa_pcd_header_xyzi_normals_binary(n, header, hcap)
                   : row_floats == 7 ? dmsa_pcd_header_normals_binary(n, header, hcap)
                   : row_floats == 4 ? dmsa_pcd_header_xyzi_binary(n, header, hcap)
                                     : dmsa_pcd_header_xyz_binary(n, header, hcap);
    if (hn < 0) return hn;
    if (!file.write(header, (size_t)hn)) return fail(ctx, DMSA_ERR_INVALID, file.why());
    const int64_t chunk = std::min(kFileChunkRows, n);
    auto rows_of = [&](int64_t c) { return std::min(chunk, n - c * chunk); };
    HIPCHK(back.create());
    for (int b = 0; b < 2; ++b) HIPCHK(back.reserve(b, (size_t)chunk * row_bytes, (size_t)chunk * row_bytes));
    auto pack = [&](int64_t c, int b) -> int {
        float* out = back.dev[b].as<float>();
        if (row_floats >= 7) launch_pack_normal_rows(dc->store.g.as<float4>(), dc->normals.normal.as<float4>(), c * chunk, rows_of(c), row_floats, out, ctx->stream);
        else launch_dense_pack_rows(dc->store.g.as<float4>() + c * chunk, words ? words + c * chunk : nullptr, rows_of(c), row_floats, out, ctx->stream);
        HIPCHK(hipGetLastError());
        return DMSA_OK;
    };
    auto bytes_of = [&](int64_t c, int, size_t* bytes) -> int { return *bytes = (size_t)rows_of(c) * row_bytes, DMSA_OK; };
    return copy_back_chunks(ctx, back, file, (n + chunk - 1) / chunk, pack, bytes_of);
}

// two fresh blocks of `rows` float4 for a store that grows or is compacted
int fresh_store(dmsa_ctx* ctx, int64_t rows, const char* what, DevBuf* g, DevBuf* o) {
    if (g->ensure((size_t)rows * 16) == hipSuccess && o->ensure((size_t)rows * 16) == hipSuccess) return DMSA_OK;
    (void)hipGetLastError();
    return fail(ctx, DMSA_ERR_NOMEM, std::string(what) + ": no device memory for a retained store of " + std::to_string(rows) + " points");
}

}  // namespace

// ---- the retained store ----
int RetainedStore::reserve(dmsa_ctx* ctx, int64_t m) {
    const int64_t need = n + m;
    if (need <= cap) return DMSA_OK;
    if (need > kMaxRetained) return fail(ctx, DMSA_ERR_NOMEM, "dense cloud: the retained store would exceed 2^31 points");
    int64_t grown = std::max<int64_t>(cap, 4096);
    while (grown < need) grown *= 2;
    grown = std::min(grown, kMaxRetained);
    DevBuf ng, no;
    CHK(fresh_store(ctx, grown, "dense cloud", &ng, &no));
    if (n > 0) {
        HIPCHK(hipMemcpyAsync(ng.p, g.p, (size_t)n * 16, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(no.p, o.p, (size_t)n * 16, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    g.swap(ng), o.swap(no);
    cap = grown;
    return DMSA_OK;  // (`ng` and `no` free the old store)
}

int RetainedStore::append(dmsa_ctx* ctx, const DevBuf& src_g, const DevBuf& src_o, int64_t m) {
    if (n + m > cap) return DMSA_ERR_INVALID;  // (never: reserve ran)
    HIPCHK(hipMemcpyAsync(g.as<float4>() + n, src_g.p, (size_t)m * 16, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(o.as<float4>() + n, src_o.p, (size_t)m * 16, hipMemcpyDeviceToDevice, ctx->stream));
    return DMSA_OK;
}

int RetainedStore::compact(dmsa_ctx* ctx, const int32_t* keep, const int32_t* scan, int64_t m, const char* what) {
    const int64_t room = std::max<int64_t>(m, 1);
    DevBuf ng, no;
    CHK(fresh_store(ctx, room, what, &ng, &no));
    launch_dense_scatter(g.as<float4>(), keep, scan, n, ng.as<float4>(), ctx->stream);
    launch_dense_scatter(o.as<float4>(), keep, scan, n, no.as<float4>(), ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    g.swap(ng), o.swap(no);
    n = m, cap = room;
    return DMSA_OK;  // (`ng` and `no` free the old store)
}

int RetainedStore::read(dmsa_ctx* ctx, int64_t first, int64_t count, float* xyz_out, float* origin_out) {
    if (xyz_out) HIPCHK(hipMemcpyAsync(xyz_out, g.as<float4>() + first, (size_t)count * 16, hipMemcpyDeviceToHost, ctx->stream));
    if (origin_out) HIPCHK(hipMemcpyAsync(origin_out, o.as<float4>() + first, (size_t)count * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

// ---- the search grid ----
int SearchGrid::build(dmsa_ctx* ctx, const float4* points, int64_t n_all, double edge_asked, const uint8_t* valid, int64_t n_valid) {
    const int64_t n = valid ? n_valid : n_all;  // the rows of the grid: those left out sort behind them
    if (rows == n && edge == edge_asked) return DMSA_OK;
    rows = 0;
    const size_t un = (size_t)n_all;
    HIPCHK(h_cells.ensure(sizeof(unsigned long long), nullptr));
    HIPCHK(cells.ensure(sizeof(unsigned long long)));
    for (DevBuf* b : {&key, &key_s}) HIPCHK(b->ensure(un * 8));
    for (DevBuf* b : {&idx, &idx_s}) HIPCHK(b->ensure(un * 4));
    HIPCHK(pts.ensure(un * 16));
    HIPCHK(sort_tmp.ensure(sort_pairs_temp_bytes(un)));
    if (valid) launch_reference_cell_keys(points, valid, n_all, edge_asked, key.as<unsigned long long>(), idx.as<uint32_t>(), ctx->stream);
    else launch_grid_cell_keys(points, n, edge_asked, key.as<unsigned long long>(), idx.as<uint32_t>(), ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(sort_pairs_u64_u32(sort_tmp.p, sort_tmp.cap, key.as<uint64_t>(), key_s.as<uint64_t>(), idx.as<uint32_t>(), idx_s.as<uint32_t>(), un, valid ? 64 : 63, 0, ctx->stream));
    unsigned long long* counter = cells.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(counter, 0, 8, ctx->stream));
    launch_grid_count_cells(key_s.as<unsigned long long>(), n, counter, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_cells.p, counter, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const uint64_t occupied = *h_cells.as<unsigned long long>();
    uint64_t slots = 1024;
    while (slots < 2 * occupied) slots <<= 1;  // never more than half full; cells <= n < 2^31
    HIPCHK(table.ensure((size_t)slots * sizeof(DenseCellEntry)));
    HIPCHK(hipMemsetAsync(table.p, 0xFF, (size_t)slots * sizeof(DenseCellEntry), ctx->stream));
    mask = (uint32_t)(slots - 1);
    launch_grid_cell_heads(points, idx_s.as<uint32_t>(), key_s.as<unsigned long long>(), n, pts.as<float4>(), table.as<DenseCellEntry>(), mask, ctx->stream);
    launch_grid_cell_ends(key_s.as<unsigned long long>(), n, table.as<DenseCellEntry>(), mask, ctx->stream);
    HIPCHK(hipGetLastError());
    rows = n, edge = edge_asked;
    return DMSA_OK;
}

// ---- a row mask ----
hipError_t RowMask::begin(int64_t n) {
    rows = -1;
    if (hipError_t e = keep.ensure((size_t)(n + 1) * 4); e != hipSuccess) return e;
    return scan.ensure((size_t)(n + 1) * 4);
}
hipError_t RowMask::enqueue_scan(int64_t n, DevBuf& scan_tmp, hipStream_t s) {
    const size_t words = (size_t)n + 1;
    if (hipError_t e = scan_tmp.ensure(scan_temp_bytes(words)); e != hipSuccess) return e;
    return exclusive_scan_i32(scan_tmp.p, scan_tmp.cap, keep.as<int32_t>(), scan.as<int32_t>(), words, s);
}

int dense_remove_rows(dmsa_dense_cloud* dc, const RowMask& mask, const char* refusal, const char* what, int64_t* kept) {
    dmsa_ctx* ctx = dc->ctx;
    if (kept) *kept = dc->store.n;
    if (!mask.valid_for(dc->store)) return fail(ctx, DMSA_ERR_INVALID, refusal);
    CHK(set_device(ctx));
    const int64_t m = mask.kept;
    CHK(dc->store.compact(ctx, mask.keep.as<int32_t>(), mask.scan.as<int32_t>(), m, what));
    store_changed(dc);  // classifications, grid and normals were of the store before
    if (kept) *kept = m;
    return DMSA_OK;
}

// ---- the preconditions ----

namespace {
int refuse(dmsa_dense_cloud* dc, const char* what, const std::string& why) { return fail(dc->ctx, DMSA_ERR_INVALID, std::string(what) + ": " + why); }
}  // namespace

int dense_retention_on(dmsa_dense_cloud* dc, const char* what) {
    return dc->store.on ? DMSA_OK : refuse(dc, what, "retention is off (dmsa_dense_cloud_retain before the first scan)");
}
int dense_store_ready(dmsa_dense_cloud* dc, const char* what) {
    CHK(dense_retention_on(dc, what));
    if (dc->store.n < 1) return refuse(dc, what, "no retained point");
    return dc->cfg.voxel_size > 0.0f ? DMSA_OK : refuse(dc, what, "voxel_size must be > 0");
}
int dense_voxel_length(dmsa_dense_cloud* dc, float x, const char* name, const char* what) {
    const float v = dc->cfg.voxel_size;
    if (!std::isfinite(x)) return refuse(dc, what, std::string(name) + " is not finite");
    return x >= v && x <= 64.0f * v ? DMSA_OK : refuse(dc, what, std::string(name) + " must lie in [voxel_size, 64 * voxel_size]");
}
int dense_row_range(dmsa_dense_cloud* dc, int64_t first, int64_t count, const char* what) {
    return first > dc->store.n || count > dc->store.n - first ? refuse(dc, what, "rows beyond the retained store") : DMSA_OK;
}
int dense_row_cap(dmsa_dense_cloud* dc, const char* what) { return dc->store.n > kMaxStageRows ? refuse(dc, what, "more than 2^26 retained rows") : DMSA_OK; }
int dense_reach_preconditions(dmsa_dense_cloud* dc, float r, const char* name, const char* what) {
    CHK(dense_store_ready(dc, what));
    CHK(dense_voxel_length(dc, r, name, what));
    return 20 - dense_radius_exponent(r) > 126 ? refuse(dc, what, std::string(name) + " is too small for the scale of N3") : DMSA_OK;
}
int dense_radius_preconditions(dmsa_dense_cloud* dc, float r, const char* what) { return dense_reach_preconditions(dc, r, "radius", what); }

// ---- the files of the store ----
int dense_save_rows(dmsa_dense_cloud* dc, const char* path, const char* what, int row_floats, int64_t* points_out, int64_t* bytes_out, RowWord word) {
    dmsa_ctx* ctx = dc->ctx;
    CHK(set_device(ctx));
    PcdFile file;
    if (!file.open(path, what)) return fail(ctx, DMSA_ERR_INVALID, file.why());
    const int rc = copy_back_end(ctx, file, write_rows(dc, file, row_floats, word));
    if (rc != DMSA_OK) return file.discard(), rc;
    if (points_out) *points_out = dc->store.n;
    if (bytes_out) *bytes_out = file.bytes();
    return DMSA_OK;
}

extern "C" {

int dmsa_dense_cloud_retain(dmsa_dense_cloud* dc) {
    if (!dc) return DMSA_ERR_INVALID;
    if (dc->scan_no != 0 || dc->total.points_in != 0) return fail(dc->ctx, DMSA_ERR_INVALID, "dense cloud: retain is legal only before the first scan is added");
    dc->store.on = true;
    return DMSA_OK;
}

int dmsa_dense_cloud_retained(dmsa_dense_cloud* dc, int64_t first, int64_t count, float* xyz_out, float* origin_out, int64_t* total_out) {
    if (total_out) *total_out = 0;
    if (!dc || first < 0 || count < 0) return DMSA_ERR_INVALID;
    CHK(dense_retention_on(dc, "dense cloud"));
    if (total_out) *total_out = dc->store.n;
    CHK(dense_row_range(dc, first, count, "dense cloud"));
    CHK(set_device(dc->ctx));
    if (count == 0) return DMSA_OK;
    return dc->store.read(dc->ctx, first, count, xyz_out, origin_out);
}

}  // extern "C"
