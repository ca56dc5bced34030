// dense_occupancy_api.cpp — include/dmsa_dense_occupancy.h on top of dense_occupancy.hip: M1's checks, the build (the search grid of the store
// with cells of cell_size for the sorted order, the table cleared, k_occupancy_walk, one small read; a table that overflowed is doubled and
// the walk run again; then the listing: flags, the library's scan, the compaction, the library's 64-bit sort, the states), the window of the
// listing, the voxel file through copy_back.h and a PcdFile, the slice and its two files, and M8.  Store, grid and the shared checks:
// dense_store.cpp (dense_cloud_obj.h).  The defaults, the host-only calls and every text: dense_occupancy_text.cpp.
#include "dense_cloud_obj.h"

#include "dense_occupancy.h"

#include <climits>
#include <cmath>
#include <vector>

namespace {

constexpr uint64_t kMaxSlots = (uint64_t)1 << 31;
constexpr int64_t kMaxPixels = (int64_t)1 << 28;
constexpr int64_t kFileChunkRows = (int64_t)1 << 20;  // 24 MiB per pinned buffer
constexpr size_t kRowBytes = 24;
constexpr int32_t kBias = 1 << 20;
const char* const kWhat = "dense occupancy";
const char* const kNoMap = "dense occupancy: no map of the store as it stands (dmsa_dense_cloud_build_occupancy first)";

// the pinned words of DenseOccupancy::h_rec
struct Readback {
    unsigned long long rec[OW_COUNT];
    unsigned long long sums[OS_STATES];
    int32_t extent[OE_COUNT];
    int32_t count;
};

OccupancyParams params_of(const dmsa_dense_occupancy_config* cfg) {
    return OccupancyParams{(double)cfg->cell_size, cfg->max_length, (uint32_t)cfg->min_hits, (uint32_t)cfg->min_passes, (uint32_t)cfg->occ_num, (uint32_t)cfg->occ_den};
}

// M1
int check_preconditions(dmsa_dense_cloud* dc, const dmsa_dense_occupancy_config* cfg) {
    CHK(dense_store_ready(dc, kWhat));
    CHK(dense_voxel_length(dc, cfg->cell_size, "cell_size", kWhat));
    const char* why = dense_occupancy_config_refusal(cfg);
    if (why) return fail(dc->ctx, DMSA_ERR_INVALID, std::string("dense occupancy: ") + why);
    return dense_row_cap(dc, kWhat);
}

// M8
int map_valid(dmsa_dense_cloud* dc) { return dc->occupancy.valid_for(dc->store) ? DMSA_OK : fail(dc->ctx, DMSA_ERR_INVALID, kNoMap); }

// the automatic first size: the smallest power of two >= 4 * rows, at least 1024
uint64_t first_slots(int64_t rows) {
    uint64_t slots = 1024;
    while (slots < 4 * (uint64_t)rows) slots <<= 1;
    return slots;
}

// M3 into a table of `slots` slots, waited for: rb->rec holds the record
int walk_once(dmsa_dense_cloud* dc, const OccupancyParams& p, uint64_t slots, Readback* rb) {
    dmsa_ctx* ctx = dc->ctx;
    DenseOccupancy& oc = dc->occupancy;
    if (oc.table.ensure((size_t)slots * sizeof(OccupancySlot)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, DMSA_ERR_NOMEM, "dense occupancy: no device memory for a table of " + std::to_string(slots) + " slots");
    }
    unsigned long long* rec = oc.rec.as<unsigned long long>();
    launch_occupancy_clear(oc.table.as<OccupancySlot>(), slots, ctx->stream);
    HIPCHK(hipMemsetAsync(rec, 0, OW_COUNT * 8, ctx->stream));
    launch_occupancy_walk(dc->shared.grid.view(), dc->store.o.as<float4>(), p, oc.table.as<OccupancySlot>(), (uint32_t)(slots - 1), slots / 2, rec, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rb->rec, rec, OW_COUNT * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

// M4-M5: the m held slots of the table listed in key order, waited for: rb->sums holds the cells of each state
int list_cells(dmsa_dense_cloud* dc, const OccupancyParams& p, uint64_t slots, int64_t m, Readback* rb) {
    dmsa_ctx* ctx = dc->ctx;
    DenseOccupancy& oc = dc->occupancy;
    const size_t um = (size_t)m, words = (size_t)slots + 1;
    unsigned long long* sums = oc.sums.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(sums, 0, OS_STATES * 8, ctx->stream));
    if (m > 0) {
        for (DevBuf* b : {&oc.flag, &oc.scan}) HIPCHK(b->ensure(words * 4));
        for (DevBuf* b : {&oc.key, &oc.key_s}) HIPCHK(b->ensure(um * 8));
        for (DevBuf* b : {&oc.slot_of, &oc.slot_s, &oc.hits, &oc.passes, &oc.state}) HIPCHK(b->ensure(um * 4));
        HIPCHK(oc.sort_tmp.ensure(sort_pairs_temp_bytes(um)));
        HIPCHK(dc->shared.scan_tmp.ensure(scan_temp_bytes(words)));
        const OccupancySlot* table = oc.table.as<OccupancySlot>();
        launch_occupancy_flags(table, slots, oc.flag.as<int32_t>(), ctx->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(exclusive_scan_i32(dc->shared.scan_tmp.p, dc->shared.scan_tmp.cap, oc.flag.as<int32_t>(), oc.scan.as<int32_t>(), words, ctx->stream));
        launch_occupancy_compact(table, slots, oc.flag.as<int32_t>(), oc.scan.as<int32_t>(), m, oc.key.as<unsigned long long>(), oc.slot_of.as<uint32_t>(), ctx->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(sort_pairs_u64_u32(oc.sort_tmp.p, oc.sort_tmp.cap, oc.key.as<uint64_t>(), oc.key_s.as<uint64_t>(), oc.slot_of.as<uint32_t>(), oc.slot_s.as<uint32_t>(), um, 63,
                                  0, ctx->stream));
        launch_occupancy_states(table, oc.slot_s.as<uint32_t>(), m, p, oc.hits.as<uint32_t>(), oc.passes.as<uint32_t>(), oc.state.as<uint32_t>(), sums, ctx->stream);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(rb->sums, sums, OS_STATES * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

// M6: header and rows of the listed cells with state >= min_state
int write_cells(dmsa_dense_cloud* dc, PcdFile& file, int32_t min_state, int64_t* rows_written) {
    dmsa_ctx* ctx = dc->ctx;
    DenseOccupancy& oc = dc->occupancy;
    CopyBack& back = dc->shared.files;
    const int64_t m = oc.cells;
    int64_t total = m;
    const uint32_t* sel = nullptr;
    if (min_state > 0 && m > 0) {  // the cells the file takes, in order
        const size_t words = (size_t)m + 1;
        Readback* rb = oc.h_rec.as<Readback>();
        for (DevBuf* b : {&oc.keep, &oc.keep_scan}) HIPCHK(b->ensure(words * 4));
        HIPCHK(oc.sel.ensure((size_t)m * 4));
        HIPCHK(dc->shared.scan_tmp.ensure(scan_temp_bytes(words)));
        launch_occupancy_select_flags(oc.state.as<uint32_t>(), m, (uint32_t)min_state, oc.keep.as<int32_t>(), ctx->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(exclusive_scan_i32(dc->shared.scan_tmp.p, dc->shared.scan_tmp.cap, oc.keep.as<int32_t>(), oc.keep_scan.as<int32_t>(), words, ctx->stream));
        launch_occupancy_select(oc.keep.as<int32_t>(), oc.keep_scan.as<int32_t>(), m, oc.sel.as<uint32_t>(), ctx->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&rb->count, oc.keep_scan.as<int32_t>() + m, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        total = rb->count, sel = oc.sel.as<uint32_t>();
        if (total < 0 || total > m) return fail(ctx, DMSA_ERR_HIP, "dense occupancy: the scan of the file's cells went wrong");  // (never)
    }
    char header[512];
    const int hn = dmsa_pcd_header_occupancy_binary(total, header, (int32_t)sizeof(header));
    if (hn < 0) return hn;
    if (!file.write(header, (size_t)hn)) return fail(ctx, DMSA_ERR_INVALID, file.why());
    if (rows_written) *rows_written = total;
    if (total == 0) return DMSA_OK;
    const int64_t chunk = std::min(kFileChunkRows, total);
    auto rows_of = [&](int64_t c) { return std::min(chunk, total - c * chunk); };
    HIPCHK(back.create());
    for (int b = 0; b < 2; ++b) HIPCHK(back.reserve(b, (size_t)chunk * kRowBytes, (size_t)chunk * kRowBytes));
    auto pack = [&](int64_t c, int b) -> int {
        launch_occupancy_rows(oc.key_s.as<unsigned long long>(), oc.hits.as<uint32_t>(), oc.passes.as<uint32_t>(), oc.state.as<uint32_t>(), sel, c * chunk, rows_of(c),
                              (double)oc.cell_size, back.dev[b].as<uint32_t>(), ctx->stream);
        HIPCHK(hipGetLastError());
        return DMSA_OK;
    };
    auto bytes_of = [&](int64_t c, int, size_t* bytes) -> int { return *bytes = (size_t)rows_of(c) * kRowBytes, DMSA_OK; };
    return copy_back_chunks(ctx, back, file, (total + chunk - 1) / chunk, pack, bytes_of);
}

// M7: the slab's image left in occupancy.pixels (info->width * info->height bytes), waited for
int slice_on_device(dmsa_dense_cloud* dc, float z_lo, float z_hi, dmsa_dense_occupancy_slice_info* info) {
    dmsa_ctx* ctx = dc->ctx;
    DenseOccupancy& oc = dc->occupancy;
    *info = dmsa_dense_occupancy_slice_info{};
    CHK(map_valid(dc));
    if (!std::isfinite(z_lo) || !std::isfinite(z_hi)) return fail(ctx, DMSA_ERR_INVALID, "dense occupancy: z_lo and z_hi must be finite");
    if (!(z_lo <= z_hi)) return fail(ctx, DMSA_ERR_INVALID, "dense occupancy: z_lo must be <= z_hi");
    const char* const empty = "dense occupancy: no map cell in the slab";
    const double c = (double)oc.cell_size;
    const double lo = std::floor((double)z_lo / c), hi = std::floor((double)z_hi / c);
    if (hi < -(double)kBias || lo > (double)(kBias - 1) || oc.cells == 0) return fail(ctx, DMSA_ERR_INVALID, empty);
    // biased, as the keys hold them
    const int32_t cz_lo = (int32_t)std::max(lo, -(double)kBias) + kBias, cz_hi = (int32_t)std::min(hi, (double)(kBias - 1)) + kBias;
    CHK(set_device(ctx));
    Readback* rb = oc.h_rec.as<Readback>();
    const int64_t m = oc.cells;
    const unsigned long long* key = oc.key_s.as<unsigned long long>();
    HIPCHK(oc.extent.ensure(OE_COUNT * 4));
    launch_occupancy_extent_init(oc.extent.as<int32_t>(), ctx->stream);
    launch_occupancy_extent(key, m, cz_lo, cz_hi, oc.extent.as<int32_t>(), ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rb->extent, oc.extent.p, OE_COUNT * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const int32_t x_min = rb->extent[OE_X_MIN], y_min = rb->extent[OE_Y_MIN], x_max = rb->extent[OE_X_MAX], y_max = rb->extent[OE_Y_MAX];
    if (x_min > x_max || y_min > y_max) return fail(ctx, DMSA_ERR_INVALID, empty);
    const int64_t width = (int64_t)x_max - x_min + 1, height = (int64_t)y_max - y_min + 1, n = width * height;
    if (n > kMaxPixels) return fail(ctx, DMSA_ERR_INVALID, "dense occupancy: the slab's image would exceed 2^28 pixels");
    unsigned long long* sums = oc.sums.as<unsigned long long>();
    HIPCHK(oc.image.ensure((size_t)n * 4));
    HIPCHK(oc.pixels.ensure((size_t)n));
    HIPCHK(hipMemsetAsync(oc.image.p, 0, (size_t)n * 4, ctx->stream));
    HIPCHK(hipMemsetAsync(sums, 0, OS_STATES * 8, ctx->stream));
    launch_occupancy_columns(key, oc.state.as<uint32_t>(), m, cz_lo, cz_hi, x_min, y_max, (int32_t)width, (int32_t)height, oc.image.as<uint32_t>(), ctx->stream);
    launch_occupancy_pixels(oc.image.as<uint32_t>(), n, oc.pixels.as<uint8_t>(), sums, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rb->sums, sums, OS_STATES * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    info->width = (int32_t)width, info->height = (int32_t)height, info->cx_min = x_min - kBias, info->cy_min = y_min - kBias;
    info->origin_x = (double)info->cx_min * c, info->origin_y = (double)info->cy_min * c;
    info->occupied = (int64_t)rb->sums[OS_OCCUPIED], info->free = (int64_t)rb->sums[OS_FREE], info->unknown = (int64_t)rb->sums[OS_UNKNOWN];
    return DMSA_OK;
}

}  // namespace

extern "C" {

int dmsa_dense_cloud_build_occupancy(dmsa_dense_cloud* dc, const dmsa_dense_occupancy_config* cfg, dmsa_dense_occupancy_stats* stats) {
    if (stats) *stats = dmsa_dense_occupancy_stats{};
    if (!dc || !cfg) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(set_device(ctx));
    DenseOccupancy& oc = dc->occupancy;
    oc.rows = -1;  // whatever fails from here on leaves no map
    const int64_t n = dc->store.n;
    const OccupancyParams p = params_of(cfg);
    CHK(dc->shared.grid.build(ctx, dc->store.g.as<float4>(), n, p.cell));
    HIPCHK(oc.rec.ensure(OW_COUNT * 8));
    HIPCHK(oc.sums.ensure(OS_STATES * 8));
    HIPCHK(oc.h_rec.ensure(sizeof(Readback), nullptr));
    Readback* rb = oc.h_rec.as<Readback>();
    uint64_t slots = cfg->initial_slots != 0 ? (uint64_t)cfg->initial_slots : first_slots(n);
    int64_t builds = 0;
    while (true) {  // (at most 26 rounds: 64 slots doubled up to 2^31)
        if (slots > kMaxSlots) return fail(ctx, DMSA_ERR_NOMEM, "dense occupancy: the table would exceed 2^31 slots");
        CHK(walk_once(dc, p, slots, rb));
        ++builds;
        if (rb->rec[OW_OVERFLOW] == 0ull) break;
        slots *= 2;
    }
    const int64_t m = (int64_t)rb->rec[OW_OCCUPIED];
    CHK(list_cells(dc, p, slots, m, rb));
    if ((int64_t)(rb->sums[OS_UNKNOWN] + rb->sums[OS_FREE] + rb->sums[OS_OCCUPIED]) != m)
        return fail(ctx, DMSA_ERR_HIP, "dense occupancy: the listing lost cells");  // (never)
    oc.rows = n, oc.cells = m, oc.cell_size = cfg->cell_size;
    if (stats) {
        stats->rows = n, stats->rays_skipped = (int64_t)rb->rec[OW_SKIPPED], stats->rays_walked = n - stats->rays_skipped;
        stats->cells_traversed = (int64_t)rb->rec[OW_CELLS], stats->cells_out_of_range = (int64_t)rb->rec[OW_OUT_OF_RANGE];
        stats->cells = m, stats->occupied = (int64_t)rb->sums[OS_OCCUPIED], stats->free = (int64_t)rb->sums[OS_FREE], stats->unknown = (int64_t)rb->sums[OS_UNKNOWN];
        stats->table_slots = (int64_t)slots, stats->table_builds = builds;
    }
    return DMSA_OK;
}

int dmsa_dense_cloud_occupancy_cells(dmsa_dense_cloud* dc, int64_t first, int64_t count, int32_t* cells_xyz, uint32_t* hits, uint32_t* passes, uint8_t* state,
                                     int64_t* total) {
    if (total) *total = 0;
    if (!dc || first < 0 || count < 0) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(map_valid(dc));
    DenseOccupancy& oc = dc->occupancy;
    if (total) *total = oc.cells;
    if (first > oc.cells || count > oc.cells - first) return fail(ctx, DMSA_ERR_INVALID, "dense occupancy: cells beyond the listing");
    if (count == 0) return DMSA_OK;
    CHK(set_device(ctx));
    const size_t un = (size_t)count;
    std::vector<unsigned long long> keys(cells_xyz ? un : 0);
    std::vector<uint32_t> states(state ? un : 0);
    if (cells_xyz) HIPCHK(hipMemcpyAsync(keys.data(), oc.key_s.as<unsigned long long>() + first, un * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (hits) HIPCHK(hipMemcpyAsync(hits, oc.hits.as<uint32_t>() + first, un * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (passes) HIPCHK(hipMemcpyAsync(passes, oc.passes.as<uint32_t>() + first, un * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (state) HIPCHK(hipMemcpyAsync(states.data(), oc.state.as<uint32_t>() + first, un * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < keys.size(); ++i) {
        const unsigned long long k = keys[i];
        cells_xyz[3 * i] = (int32_t)((k >> 42) & 0x1FFFFFull) - kBias, cells_xyz[3 * i + 1] = (int32_t)((k >> 21) & 0x1FFFFFull) - kBias;
        cells_xyz[3 * i + 2] = (int32_t)(k & 0x1FFFFFull) - kBias;
    }
    for (size_t i = 0; i < states.size(); ++i) state[i] = (uint8_t)states[i];
    return DMSA_OK;
}

int dmsa_dense_cloud_save_pcd_occupancy(dmsa_dense_cloud* dc, const char* path, int32_t min_state, int64_t* rows_written) {
    if (rows_written) *rows_written = 0;
    if (!dc || !path) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(map_valid(dc));
    if (min_state < 0 || min_state > 2) return fail(ctx, DMSA_ERR_INVALID, "dense occupancy: min_state must lie in [0, 2]");
    CHK(set_device(ctx));
    PcdFile file;
    if (!file.open(path, kWhat)) return fail(ctx, DMSA_ERR_INVALID, file.why());
    int64_t rows = 0;
    const int rc = copy_back_end(ctx, file, write_cells(dc, file, min_state, &rows));
    if (rc != DMSA_OK) return file.discard(), rc;
    if (rows_written) *rows_written = rows;
    return DMSA_OK;
}

int dmsa_dense_cloud_occupancy_slice(dmsa_dense_cloud* dc, float z_lo, float z_hi, dmsa_dense_occupancy_slice_info* info, uint8_t* pixels, int64_t cap) {
    if (info) *info = dmsa_dense_occupancy_slice_info{};
    if (!dc || !info || cap < 0 || (cap > 0 && !pixels)) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(slice_on_device(dc, z_lo, z_hi, info));
    if (!pixels) return DMSA_OK;
    const int64_t n = (int64_t)info->width * info->height;
    if (cap < n) return fail(ctx, DMSA_ERR_INVALID, "dense occupancy: pixels holds fewer than width * height bytes");
    HIPCHK(hipMemcpyAsync(pixels, dc->occupancy.pixels.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

int dmsa_dense_cloud_save_occupancy_map(dmsa_dense_cloud* dc, const char* pgm_path, const char* yaml_path, float z_lo, float z_hi) {
    if (!dc || !pgm_path || !yaml_path) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    dmsa_dense_occupancy_slice_info info;
    CHK(slice_on_device(dc, z_lo, z_hi, &info));
    const size_t n = (size_t)info.width * (size_t)info.height;
    std::vector<uint8_t> pixels(n);
    HIPCHK(hipMemcpyAsync(pixels.data(), dc->occupancy.pixels.p, n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    char head[64], yaml[4608];
    const int hn = dmsa_occupancy_map_pgm_header(info.width, info.height, head, (int32_t)sizeof(head));
    const int yn = dmsa_occupancy_map_yaml(pgm_path, dc->occupancy.cell_size, info.cx_min, info.cy_min, yaml, (int32_t)sizeof(yaml));
    if (hn < 0 || yn < 0) return fail(ctx, DMSA_ERR_INVALID, "dense occupancy: the pgm path is too long for the yaml text");
    PcdFile pgm, text;
    if (!pgm.open(pgm_path, kWhat)) return fail(ctx, DMSA_ERR_INVALID, pgm.why());
    if (!pgm.write(head, (size_t)hn) || !pgm.write(pixels.data(), n) || !pgm.close()) return pgm.discard(), fail(ctx, DMSA_ERR_INVALID, pgm.why());
    if (!text.open(yaml_path, kWhat)) return pgm.discard(), fail(ctx, DMSA_ERR_INVALID, text.why());
    if (!text.write(yaml, (size_t)yn) || !text.close()) return pgm.discard(), text.discard(), fail(ctx, DMSA_ERR_INVALID, text.why());
    return DMSA_OK;
}

}  // extern "C"
