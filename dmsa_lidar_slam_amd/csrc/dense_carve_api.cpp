// dense_carve_api.cpp — include/dmsa_dense_carve.h on top of dense_carve.hip: T1's checks, the stage call of the walk, the launch sequence of a
// count (the grid of dense_normals_api.cpp with cells of cell_size, k_carve_passes, the flags and their scan, one host read of the statistics)
// and the removal (T7: dense_compact_store of dense_cloud_obj.h).  The defaults and the two host-only calls: dense_carve_text.cpp.
#include "dense_cloud_obj.h"

#include "dense_carve.h"

namespace {

constexpr int64_t kMaxCarveRows = (int64_t)1 << 26;  // T1

CarveParams params_of(const dmsa_dense_carve_config* cfg) {
    return CarveParams{(double)cfg->cell_size, cfg->rho, cfg->tan_half_angle, cfg->end_margin, cfg->start_margin, cfg->max_length};
}

// T1
int check_preconditions(dmsa_dense_cloud* dc, const dmsa_dense_carve_config* cfg) {
    dmsa_ctx* ctx = dc->ctx;
    if (!dc->retain) return fail(ctx, DMSA_ERR_INVALID, "dense carve: retention is off (dmsa_dense_cloud_retain before the first scan)");
    if (dc->ret_n < 1) return fail(ctx, DMSA_ERR_INVALID, "dense carve: no retained point");
    const float v = dc->cfg.voxel_size;
    if (!(v > 0.0f)) return fail(ctx, DMSA_ERR_INVALID, "dense carve: voxel_size must be > 0");
    if (!std::isfinite(cfg->cell_size)) return fail(ctx, DMSA_ERR_INVALID, "dense carve: cell_size is not finite");
    if (!(cfg->cell_size >= v && cfg->cell_size <= 64.0f * v)) return fail(ctx, DMSA_ERR_INVALID, "dense carve: cell_size must lie in [voxel_size, 64 * voxel_size]");
    const char* why = dense_carve_config_refusal(cfg);
    if (why) return fail(ctx, DMSA_ERR_INVALID, std::string("dense carve: ") + why);
    if (dc->ret_n > kMaxCarveRows) return fail(ctx, DMSA_ERR_INVALID, "dense carve: more than 2^26 retained rows");
    return DMSA_OK;
}

}  // namespace

extern "C" {

int dmsa_dense_cloud_carve_walk_rows(dmsa_dense_cloud* dc, const dmsa_dense_carve_config* cfg, int64_t first, int64_t count, int32_t* n_cells, uint64_t* cell_hash) {
    if (!dc || !cfg || first < 0 || count < 0) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    if (first > dc->ret_n || count > dc->ret_n - first) return fail(ctx, DMSA_ERR_INVALID, "dense carve: rows beyond the retained store");
    if (count == 0) return DMSA_OK;
    CHK(set_device(ctx));
    DenseNormalsState* st = nullptr;
    CHK(dense_normals_state(dc, &st));
    HIPCHK(st->walk_cells.ensure((size_t)count * 4));
    HIPCHK(st->walk_hash.ensure((size_t)count * 8));
    launch_carve_walk_rows(dc->ret_g.as<float4>(), dc->ret_o.as<float4>(), first, count, params_of(cfg), st->walk_cells.as<int32_t>(),
                           st->walk_hash.as<unsigned long long>(), ctx->stream);
    HIPCHK(hipGetLastError());
    if (n_cells) HIPCHK(hipMemcpyAsync(n_cells, st->walk_cells.p, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (cell_hash) HIPCHK(hipMemcpyAsync(cell_hash, st->walk_hash.p, (size_t)count * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

int dmsa_dense_cloud_count_passes(dmsa_dense_cloud* dc, const dmsa_dense_carve_config* cfg, uint32_t* passes_out, dmsa_dense_carve_stats* stats) {
    if (stats) *stats = dmsa_dense_carve_stats{};
    if (!dc || !cfg) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(set_device(ctx));
    DenseNormalsState* st = nullptr;
    CHK(dense_normals_state(dc, &st));
    st->carve_n = -1;
    const int64_t n = dc->ret_n;
    const size_t un = (size_t)n;
    CHK(dense_normals_grid(dc, st, (double)cfg->cell_size));
    HIPCHK(st->passes.ensure(un * 4));
    HIPCHK(st->carve_keep.ensure((un + 1) * 4));
    HIPCHK(st->carve_scan.ensure((un + 1) * 4));
    HIPCHK(st->scan_tmp.ensure(scan_temp_bytes(un + 1)));
    HIPCHK(st->carve_sums.ensure(CS_COUNT * 8));
    HIPCHK(st->h_carve.ensure(CS_COUNT * 8 + 8, nullptr));
    unsigned long long* sums = st->carve_sums.as<unsigned long long>();
    unsigned long long* h = st->h_carve.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(sums, 0, CS_COUNT * 8, ctx->stream));
    HIPCHK(hipMemsetAsync(st->passes.p, 0, un * 4, ctx->stream));
    launch_carve_passes(st->pts.as<float4>(), st->idx_s.as<uint32_t>(), dc->ret_o.as<float4>(), n, st->table.as<DenseCellEntry>(), st->mask, params_of(cfg),
                        st->passes.as<uint32_t>(), sums, ctx->stream);
    launch_carve_flags(st->passes.as<uint32_t>(), n, (uint32_t)cfg->min_passes, st->carve_keep.as<int32_t>(), ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(exclusive_scan_i32(st->scan_tmp.p, st->scan_tmp.cap, st->carve_keep.as<int32_t>(), st->carve_scan.as<int32_t>(), un + 1, ctx->stream));
    int32_t* h_kept = reinterpret_cast<int32_t*>(h + CS_COUNT);
    HIPCHK(hipMemcpyAsync(h, sums, CS_COUNT * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h_kept, st->carve_scan.as<int32_t>() + n, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (passes_out) HIPCHK(hipMemcpyAsync(passes_out, st->passes.p, un * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // the one host read
    st->carve_n = n;
    if (stats) {
        stats->rows = n, stats->rays_skipped = (int64_t)h[CS_SKIPPED], stats->rays_walked = n - stats->rays_skipped;
        stats->cells_traversed = (int64_t)h[CS_CELLS], stats->pair_tests = (int64_t)h[CS_PAIRS], stats->seen_through = (int64_t)h[CS_SEEN];
        stats->kept = *h_kept, stats->transient = n - stats->kept;
    }
    return DMSA_OK;
}

int dmsa_dense_cloud_remove_transients(dmsa_dense_cloud* dc, int64_t* kept) {
    if (kept) *kept = 0;
    if (!dc) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    DenseNormalsState* st = dc->nrm;
    if (kept) *kept = dc->ret_n;
    if (!dc->retain || !st || st->carve_n < 0 || st->carve_n != dc->ret_n)
        return fail(ctx, DMSA_ERR_INVALID, "dense carve: no pass counts of the store as it stands (dmsa_dense_cloud_count_passes first)");
    CHK(set_device(ctx));
    const int64_t m = *reinterpret_cast<int32_t*>(st->h_carve.as<unsigned long long>() + CS_COUNT);
    CHK(dense_compact_store(dc, st->carve_keep.as<int32_t>(), st->carve_scan.as<int32_t>(), m, "dense carve"));
    if (kept) *kept = m;
    return DMSA_OK;
}

}  // extern "C"
