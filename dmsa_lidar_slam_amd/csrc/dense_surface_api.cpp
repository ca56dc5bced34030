// dense_surface_api.cpp — include/dmsa_dense_surface.h on top of dense_surface.hip: S1's checks, the build (the search grid of the store with
// cells of cell_size for the sorted order, the table cleared, k_surface_integrate, one small read; a table that overflowed is doubled and the
// walk run again; then the listing: flags, the library's scan, the compaction, the library's 64-bit sort, sums and weights in order and every
// cell's index back into its slot), the window of the listing, the voxel file through copy_back.h and a PcdFile, the extraction (mark, count,
// one small read, the two scans, emit), the windows of the mesh, the PLY through the same pipeline, and S10.  Store, grid and the shared
// checks: dense_store.cpp (dense_cloud_obj.h).  The defaults, the host-only calls and both headers: dense_surface_text.cpp.
#include "dense_cloud_obj.h"

#include "dense_surface.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace {

constexpr uint64_t kMaxSlots = (uint64_t)1 << 31;
constexpr int64_t kMaxMeshCount = 2147483647ll;       // S8: vertices, triangles
constexpr int64_t kFileChunkRows = (int64_t)1 << 20;  // at most 20 MiB per pinned buffer
constexpr size_t kCellRowBytes = 20, kVertexRowBytes = 12, kFaceRowBytes = 13;
constexpr int32_t kBias = 1 << 20;
const char* const kWhat = "dense surface";
const char* const kNoVolume = "dense surface: no volume of the store as it stands (dmsa_dense_cloud_build_surface first)";
const char* const kNoMesh = "dense surface: no mesh of the volume as it stands (dmsa_dense_cloud_extract_mesh first)";

// the pinned words of DenseSurface::h_rec
struct Readback {
    unsigned long long rec[SW_COUNT];
    unsigned long long mesh[MW_COUNT];
};

SurfaceParams params_of(const dmsa_dense_surface_config* cfg) { return SurfaceParams{(double)cfg->cell_size, cfg->truncation, cfg->max_length}; }

// S1
int check_preconditions(dmsa_dense_cloud* dc, const dmsa_dense_surface_config* cfg) {
    CHK(dense_store_ready(dc, kWhat));
    CHK(dense_voxel_length(dc, cfg->cell_size, "cell_size", kWhat));
    const char* why = dense_surface_config_refusal(cfg);
    if (why) return fail(dc->ctx, DMSA_ERR_INVALID, std::string("dense surface: ") + why);
    return dense_row_cap(dc, kWhat);
}

// S10
int volume_valid(dmsa_dense_cloud* dc) { return dc->surface.valid_for(dc->store) ? DMSA_OK : fail(dc->ctx, DMSA_ERR_INVALID, kNoVolume); }
int mesh_valid(dmsa_dense_cloud* dc) {
    CHK(volume_valid(dc));
    return dc->surface.mesh_valid_for(dc->store) ? DMSA_OK : fail(dc->ctx, DMSA_ERR_INVALID, kNoMesh);
}

// the automatic first size: the smallest power of two >= 4 * rows, at least 1024
uint64_t first_slots(int64_t rows) {
    uint64_t slots = 1024;
    while (slots < 4 * (uint64_t)rows) slots <<= 1;
    return slots;
}

// S2-S5 into a table of `slots` slots, waited for: rb->rec holds the record
int integrate_once(dmsa_dense_cloud* dc, const SurfaceParams& p, uint64_t slots, Readback* rb) {
    dmsa_ctx* ctx = dc->ctx;
    DenseSurface& sf = dc->surface;
    if (sf.table.ensure((size_t)slots * sizeof(SurfaceSlot)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, DMSA_ERR_NOMEM, "dense surface: no device memory for a table of " + std::to_string(slots) + " slots");
    }
    unsigned long long* rec = sf.rec.as<unsigned long long>();
    launch_surface_clear(sf.table.as<SurfaceSlot>(), slots, ctx->stream);
    HIPCHK(hipMemsetAsync(rec, 0, SW_COUNT * 8, ctx->stream));
    launch_surface_integrate(dc->shared.grid.view(), dc->store.o.as<float4>(), p, sf.table.as<SurfaceSlot>(), (uint32_t)(slots - 1), slots / 2, rec, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rb->rec, rec, SW_COUNT * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

// S6: the m held slots of the table listed in key order, waited for: rb->rec[SW_VALID] holds the cells with n >= min_weight
int list_cells(dmsa_dense_cloud* dc, uint64_t slots, int64_t m, uint32_t min_weight, Readback* rb) {
    dmsa_ctx* ctx = dc->ctx;
    DenseSurface& sf = dc->surface;
    const size_t um = (size_t)m, words = (size_t)slots + 1;
    unsigned long long* rec = sf.rec.as<unsigned long long>();
    if (m > 0) {
        for (DevBuf* b : {&sf.flag, &sf.scan}) HIPCHK(b->ensure(words * 4));
        for (DevBuf* b : {&sf.key, &sf.key_s, &sf.sum}) HIPCHK(b->ensure(um * 8));
        for (DevBuf* b : {&sf.slot_of, &sf.slot_s, &sf.weight}) HIPCHK(b->ensure(um * 4));
        HIPCHK(sf.sort_tmp.ensure(sort_pairs_temp_bytes(um)));
        HIPCHK(dc->shared.scan_tmp.ensure(scan_temp_bytes(words)));
        SurfaceSlot* table = sf.table.as<SurfaceSlot>();
        launch_surface_flags(table, slots, sf.flag.as<int32_t>(), ctx->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(exclusive_scan_i32(dc->shared.scan_tmp.p, dc->shared.scan_tmp.cap, sf.flag.as<int32_t>(), sf.scan.as<int32_t>(), words, ctx->stream));
        launch_surface_compact(table, slots, sf.flag.as<int32_t>(), sf.scan.as<int32_t>(), m, sf.key.as<unsigned long long>(), sf.slot_of.as<uint32_t>(), ctx->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(sort_pairs_u64_u32(sf.sort_tmp.p, sf.sort_tmp.cap, sf.key.as<uint64_t>(), sf.key_s.as<uint64_t>(), sf.slot_of.as<uint32_t>(), sf.slot_s.as<uint32_t>(), um, 63,
                                  0, ctx->stream));
        launch_surface_list(table, sf.slot_s.as<uint32_t>(), m, min_weight, sf.sum.as<long long>(), sf.weight.as<uint32_t>(), rec, ctx->stream);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(rb->rec, rec, SW_COUNT * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

SurfaceVolume volume_of(const DenseSurface& sf) {
    return SurfaceVolume{sf.key_s.as<unsigned long long>(), sf.sum.as<long long>(), sf.weight.as<uint32_t>(), sf.cells, sf.table.as<SurfaceSlot>(), (uint32_t)(sf.slots - 1),
                         (double)sf.cell_size};
}

// S7: header and rows of the listed cells
int write_cells(dmsa_dense_cloud* dc, PcdFile& file) {
    dmsa_ctx* ctx = dc->ctx;
    DenseSurface& sf = dc->surface;
    CopyBack& back = dc->shared.files;
    const int64_t total = sf.cells;
    char header[512];
    const int hn = dmsa_pcd_header_tsdf_binary(total, header, (int32_t)sizeof(header));
    if (hn < 0) return hn;
    if (!file.write(header, (size_t)hn)) return fail(ctx, DMSA_ERR_INVALID, file.why());
    if (total == 0) return DMSA_OK;
    const int64_t chunk = std::min(kFileChunkRows, total);
    auto rows_of = [&](int64_t c) { return std::min(chunk, total - c * chunk); };
    HIPCHK(back.create());
    for (int b = 0; b < 2; ++b) HIPCHK(back.reserve(b, (size_t)chunk * kCellRowBytes, (size_t)chunk * kCellRowBytes));
    auto pack = [&](int64_t c, int b) -> int {
        launch_surface_rows(sf.key_s.as<unsigned long long>(), sf.sum.as<long long>(), sf.weight.as<uint32_t>(), c * chunk, rows_of(c), (double)sf.cell_size, sf.truncation,
                            back.dev[b].as<uint32_t>(), ctx->stream);
        HIPCHK(hipGetLastError());
        return DMSA_OK;
    };
    auto bytes_of = [&](int64_t c, int, size_t* bytes) -> int { return *bytes = (size_t)rows_of(c) * kCellRowBytes, DMSA_OK; };
    return copy_back_chunks(ctx, back, file, (total + chunk - 1) / chunk, pack, bytes_of);
}

// S9: header, then the vertex rows as they lie in HBM, then the face rows packed chunk by chunk
int write_mesh(dmsa_dense_cloud* dc, PcdFile& file) {
    dmsa_ctx* ctx = dc->ctx;
    DenseSurface& sf = dc->surface;
    CopyBack& back = dc->shared.files;
    const int64_t nv = sf.vertices, nt = sf.triangles;
    char header[512];
    const int hn = dmsa_ply_header_mesh(nv, nt, header, (int32_t)sizeof(header));
    if (hn < 0) return hn;
    if (!file.write(header, (size_t)hn)) return fail(ctx, DMSA_ERR_INVALID, file.why());
    if (nv == 0 && nt == 0) return DMSA_OK;
    const int64_t chunk = kFileChunkRows;
    const int64_t v_chunks = (nv + chunk - 1) / chunk, t_chunks = (nt + chunk - 1) / chunk;
    HIPCHK(back.create());
    for (int b = 0; b < 2; ++b) HIPCHK(back.reserve(b, (size_t)std::min(chunk, std::max(nv, nt)) * kFaceRowBytes, (size_t)std::min(chunk, std::max(nv, nt)) * kFaceRowBytes));
    // chunk c: vertex rows while c < v_chunks, face rows after
    auto rows_of = [&](int64_t c) { return c < v_chunks ? std::min(chunk, nv - c * chunk) : std::min(chunk, nt - (c - v_chunks) * chunk); };
    auto pack = [&](int64_t c, int b) -> int {
        if (c < v_chunks) {
            HIPCHK(hipMemcpyAsync(back.dev[b].p, sf.xyz.as<float>() + 3 * c * chunk, (size_t)rows_of(c) * kVertexRowBytes, hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            launch_mesh_face_rows(sf.indices.as<int32_t>(), (c - v_chunks) * chunk, rows_of(c), back.dev[b].as<uint8_t>(), ctx->stream);
            HIPCHK(hipGetLastError());
        }
        return DMSA_OK;
    };
    auto bytes_of = [&](int64_t c, int, size_t* bytes) -> int { return *bytes = (size_t)rows_of(c) * (c < v_chunks ? kVertexRowBytes : kFaceRowBytes), DMSA_OK; };
    return copy_back_chunks(ctx, back, file, v_chunks + t_chunks, pack, bytes_of);
}

// a window [first, first + count) of `total` items
int window(dmsa_dense_cloud* dc, int64_t first, int64_t count, int64_t total, const char* beyond) {
    return first > total || count > total - first ? fail(dc->ctx, DMSA_ERR_INVALID, beyond) : DMSA_OK;
}

}  // namespace

extern "C" {

int dmsa_dense_cloud_build_surface(dmsa_dense_cloud* dc, const dmsa_dense_surface_config* cfg, dmsa_dense_surface_stats* stats) {
    if (stats) *stats = dmsa_dense_surface_stats{};
    if (!dc || !cfg) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(set_device(ctx));
    DenseSurface& sf = dc->surface;
    sf.rows = -1, sf.vertices = -1;  // whatever fails from here on leaves neither volume nor mesh
    const int64_t n = dc->store.n;
    const SurfaceParams p = params_of(cfg);
    CHK(dc->shared.grid.build(ctx, dc->store.g.as<float4>(), n, p.cell));
    HIPCHK(sf.rec.ensure(SW_COUNT * 8));
    HIPCHK(sf.h_rec.ensure(sizeof(Readback), nullptr));
    Readback* rb = sf.h_rec.as<Readback>();
    uint64_t slots = cfg->initial_slots != 0 ? (uint64_t)cfg->initial_slots : first_slots(n);
    int64_t builds = 0;
    while (true) {  // (at most 26 rounds: 64 slots doubled up to 2^31)
        if (slots > kMaxSlots) return fail(ctx, DMSA_ERR_NOMEM, "dense surface: the table would exceed 2^31 slots");
        CHK(integrate_once(dc, p, slots, rb));
        ++builds;
        if (rb->rec[SW_OVERFLOW] == 0ull) break;
        slots *= 2;
    }
    const int64_t m = (int64_t)rb->rec[SW_OCCUPIED];
    CHK(list_cells(dc, slots, m, (uint32_t)cfg->min_weight, rb));
    sf.rows = n, sf.cells = m, sf.slots = slots, sf.cell_size = cfg->cell_size, sf.truncation = cfg->truncation;
    if (stats) {
        stats->rows = n, stats->rays_skipped = (int64_t)rb->rec[SW_SKIPPED], stats->rays_walked = n - stats->rays_skipped;
        stats->cells_traversed = (int64_t)rb->rec[SW_CELLS], stats->cells_out_of_range = (int64_t)rb->rec[SW_OUT_OF_RANGE];
        stats->cells = m, stats->cells_valid = (int64_t)rb->rec[SW_VALID];
        stats->table_slots = (int64_t)slots, stats->table_builds = builds;
    }
    return DMSA_OK;
}

int dmsa_dense_cloud_surface_cells(dmsa_dense_cloud* dc, int64_t first, int64_t count, int32_t* cells_xyz, int64_t* sum, uint32_t* n, int64_t* total) {
    if (total) *total = 0;
    if (!dc || first < 0 || count < 0) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(volume_valid(dc));
    DenseSurface& sf = dc->surface;
    if (total) *total = sf.cells;
    CHK(window(dc, first, count, sf.cells, "dense surface: cells beyond the listing"));
    if (count == 0) return DMSA_OK;
    CHK(set_device(ctx));
    const size_t un = (size_t)count;
    std::vector<unsigned long long> keys(cells_xyz ? un : 0);
    if (cells_xyz) HIPCHK(hipMemcpyAsync(keys.data(), sf.key_s.as<unsigned long long>() + first, un * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (sum) HIPCHK(hipMemcpyAsync(sum, sf.sum.as<long long>() + first, un * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (n) HIPCHK(hipMemcpyAsync(n, sf.weight.as<uint32_t>() + first, un * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < keys.size(); ++i) {
        const unsigned long long k = keys[i];
        cells_xyz[3 * i] = (int32_t)((k >> 42) & 0x1FFFFFull) - kBias, cells_xyz[3 * i + 1] = (int32_t)((k >> 21) & 0x1FFFFFull) - kBias;
        cells_xyz[3 * i + 2] = (int32_t)(k & 0x1FFFFFull) - kBias;
    }
    return DMSA_OK;
}

int dmsa_dense_cloud_save_pcd_tsdf(dmsa_dense_cloud* dc, const char* path, int64_t* rows_written) {
    if (rows_written) *rows_written = 0;
    if (!dc || !path) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(volume_valid(dc));
    CHK(set_device(ctx));
    PcdFile file;
    if (!file.open(path, kWhat)) return fail(ctx, DMSA_ERR_INVALID, file.why());
    const int rc = copy_back_end(ctx, file, write_cells(dc, file));
    if (rc != DMSA_OK) return file.discard(), rc;
    if (rows_written) *rows_written = dc->surface.cells;
    return DMSA_OK;
}

int dmsa_dense_cloud_extract_mesh(dmsa_dense_cloud* dc, int32_t min_weight, dmsa_dense_mesh_stats* stats) {
    if (stats) *stats = dmsa_dense_mesh_stats{};
    if (!dc) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(volume_valid(dc));
    if (const char* why = dense_surface_weight_refusal(min_weight)) return fail(ctx, DMSA_ERR_INVALID, std::string("dense surface: ") + why);
    CHK(set_device(ctx));
    DenseSurface& sf = dc->surface;
    sf.vertices = -1;  // whatever fails from here on leaves no mesh
    const int64_t m = sf.cells;
    const size_t words = (size_t)m + 1;
    Readback* rb = sf.h_rec.as<Readback>();
    HIPCHK(sf.sums.ensure(MW_COUNT * 8));
    unsigned long long* sums = sf.sums.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(sums, 0, MW_COUNT * 8, ctx->stream));
    if (m > 0) {
        const SurfaceVolume v = volume_of(sf);
        HIPCHK(sf.used.ensure((size_t)m * kMeshClasses));
        for (DevBuf* b : {&sf.tris, &sf.verts, &sf.tri_scan, &sf.vert_scan}) HIPCHK(b->ensure(words * 4));
        HIPCHK(dc->shared.scan_tmp.ensure(scan_temp_bytes(words)));
        HIPCHK(hipMemsetAsync(sf.used.p, 0, (size_t)m * kMeshClasses, ctx->stream));
        launch_mesh_mark(v, (uint32_t)min_weight, sf.tris.as<int32_t>(), sf.used.as<uint8_t>(), sums, ctx->stream);
        launch_mesh_count(sf.used.as<uint8_t>(), m, sf.verts.as<int32_t>(), sums, ctx->stream);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(rb->mesh, sums, MW_COUNT * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const int64_t nv = (int64_t)rb->mesh[MW_VERTICES], nt = (int64_t)rb->mesh[MW_TRIANGLES];
    if (nv > kMaxMeshCount || nt > kMaxMeshCount) return fail(ctx, DMSA_ERR_INVALID, "dense surface: the mesh would exceed 2^31 - 1 vertices or triangles");
    if (nt > 0) {  // (the counts fit an int32, so do their scans)
        HIPCHK(sf.xyz.ensure((size_t)nv * 12));
        HIPCHK(sf.indices.ensure((size_t)nt * 12));
        HIPCHK(exclusive_scan_i32(dc->shared.scan_tmp.p, dc->shared.scan_tmp.cap, sf.tris.as<int32_t>(), sf.tri_scan.as<int32_t>(), words, ctx->stream));
        HIPCHK(exclusive_scan_i32(dc->shared.scan_tmp.p, dc->shared.scan_tmp.cap, sf.verts.as<int32_t>(), sf.vert_scan.as<int32_t>(), words, ctx->stream));
        launch_mesh_emit(volume_of(sf), (uint32_t)min_weight, surface_orientation(), sf.used.as<uint8_t>(), sf.vert_scan.as<int32_t>(), sf.tri_scan.as<int32_t>(), nv, nt,
                         sf.xyz.as<float>(), sf.indices.as<int32_t>(), ctx->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    sf.vertices = nv, sf.triangles = nt;
    if (stats) stats->tetrahedra_meshed = (int64_t)rb->mesh[MW_TETRAHEDRA], stats->vertices = nv, stats->triangles = nt;
    return DMSA_OK;
}

int dmsa_dense_cloud_mesh_vertices(dmsa_dense_cloud* dc, int64_t first, int64_t count, float* xyz, int64_t* total) {
    if (total) *total = 0;
    if (!dc || first < 0 || count < 0) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(mesh_valid(dc));
    DenseSurface& sf = dc->surface;
    if (total) *total = sf.vertices;
    CHK(window(dc, first, count, sf.vertices, "dense surface: vertices beyond the mesh"));
    if (count == 0 || !xyz) return DMSA_OK;
    CHK(set_device(ctx));
    HIPCHK(hipMemcpyAsync(xyz, sf.xyz.as<float>() + 3 * first, (size_t)count * 12, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

int dmsa_dense_cloud_mesh_triangles(dmsa_dense_cloud* dc, int64_t first, int64_t count, int32_t* indices, int64_t* total) {
    if (total) *total = 0;
    if (!dc || first < 0 || count < 0) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(mesh_valid(dc));
    DenseSurface& sf = dc->surface;
    if (total) *total = sf.triangles;
    CHK(window(dc, first, count, sf.triangles, "dense surface: triangles beyond the mesh"));
    if (count == 0 || !indices) return DMSA_OK;
    CHK(set_device(ctx));
    HIPCHK(hipMemcpyAsync(indices, sf.indices.as<int32_t>() + 3 * first, (size_t)count * 12, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

int dmsa_dense_cloud_save_ply_mesh(dmsa_dense_cloud* dc, const char* path) {
    if (!dc || !path) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(mesh_valid(dc));
    CHK(set_device(ctx));
    PcdFile file;
    if (!file.open(path, kWhat)) return fail(ctx, DMSA_ERR_INVALID, file.why());
    const int rc = copy_back_end(ctx, file, write_mesh(dc, file));
    if (rc != DMSA_OK) return file.discard(), rc;
    return DMSA_OK;
}

}  // extern "C"
