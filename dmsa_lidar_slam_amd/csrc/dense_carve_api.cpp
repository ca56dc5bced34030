// dense_carve_api.cpp — include/dmsa_dense_carve.h on top of dense_carve.hip: T1's checks, the stage call of the walk, the launch sequence of a
// count (the search grid of the store with cells of cell_size, k_carve_passes, the flags and their scan into the stage's row mask, one host
// read of the statistics) and the removal by that mask (T7).  Store, grid, mask and the shared checks: dense_store.cpp (dense_cloud_obj.h).
// The defaults and the two host-only calls: dense_carve_text.cpp.
#include "dense_cloud_obj.h"

#include "dense_carve.h"

namespace {

CarveParams params_of(const dmsa_dense_carve_config* cfg) {
    return CarveParams{(double)cfg->cell_size, cfg->rho, cfg->tan_half_angle, cfg->end_margin, cfg->start_margin, cfg->max_length};
}

// T1
int check_preconditions(dmsa_dense_cloud* dc, const dmsa_dense_carve_config* cfg) {
    CHK(dense_store_ready(dc, "dense carve"));
    CHK(dense_voxel_length(dc, cfg->cell_size, "cell_size", "dense carve"));
    const char* why = dense_carve_config_refusal(cfg);
    if (why) return fail(dc->ctx, DMSA_ERR_INVALID, std::string("dense carve: ") + why);
    return dense_row_cap(dc, "dense carve");
}

}  // namespace

extern "C" {

int dmsa_dense_cloud_carve_walk_rows(dmsa_dense_cloud* dc, const dmsa_dense_carve_config* cfg, int64_t first, int64_t count, int32_t* n_cells, uint64_t* cell_hash) {
    if (!dc || !cfg || first < 0 || count < 0) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(dense_row_range(dc, first, count, "dense carve"));
    if (count == 0) return DMSA_OK;
    CHK(set_device(ctx));
    DenseCarve& cv = dc->carve;
    HIPCHK(cv.walk_cells.ensure((size_t)count * 4));
    HIPCHK(cv.walk_hash.ensure((size_t)count * 8));
    launch_carve_walk_rows(dc->store.g.as<float4>(), dc->store.o.as<float4>(), first, count, params_of(cfg), cv.walk_cells.as<int32_t>(),
                           cv.walk_hash.as<unsigned long long>(), ctx->stream);
    HIPCHK(hipGetLastError());
    if (n_cells) HIPCHK(hipMemcpyAsync(n_cells, cv.walk_cells.p, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (cell_hash) HIPCHK(hipMemcpyAsync(cell_hash, cv.walk_hash.p, (size_t)count * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

int dmsa_dense_cloud_count_passes(dmsa_dense_cloud* dc, const dmsa_dense_carve_config* cfg, uint32_t* passes_out, dmsa_dense_carve_stats* stats) {
    if (stats) *stats = dmsa_dense_carve_stats{};
    if (!dc || !cfg) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(set_device(ctx));
    DenseCarve& cv = dc->carve;
    SearchGrid& grid = dc->shared.grid;
    const int64_t n = dc->store.n;
    const size_t un = (size_t)n;
    HIPCHK(cv.mask.begin(n));
    CHK(grid.build(ctx, dc->store.g.as<float4>(), dc->store.n, (double)cfg->cell_size));
    HIPCHK(cv.passes.ensure(un * 4));
    HIPCHK(cv.sums.ensure(CS_COUNT * 8));
    HIPCHK(cv.h_sums.ensure(CS_COUNT * 8 + 8, nullptr));
    unsigned long long* sums = cv.sums.as<unsigned long long>();
    unsigned long long* h = cv.h_sums.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(sums, 0, CS_COUNT * 8, ctx->stream));
    HIPCHK(hipMemsetAsync(cv.passes.p, 0, un * 4, ctx->stream));
    launch_carve_passes(grid.view(), dc->store.o.as<float4>(), params_of(cfg), cv.passes.as<uint32_t>(), sums, ctx->stream);
    launch_carve_flags(cv.passes.as<uint32_t>(), n, (uint32_t)cfg->min_passes, cv.mask.keep.as<int32_t>(), ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(cv.mask.enqueue_scan(n, dc->shared.scan_tmp, ctx->stream));
    HIPCHK(hipMemcpyAsync(h, sums, CS_COUNT * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(cv.mask.enqueue_count(n, cv.h_sums.as<int32_t>() + 2 * CS_COUNT, ctx->stream));
    if (passes_out) HIPCHK(hipMemcpyAsync(passes_out, cv.passes.p, un * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // the one host read
    cv.mask.commit(n);
    if (stats) {
        stats->rows = n, stats->rays_skipped = (int64_t)h[CS_SKIPPED], stats->rays_walked = n - stats->rays_skipped;
        stats->cells_traversed = (int64_t)h[CS_CELLS], stats->pair_tests = (int64_t)h[CS_PAIRS], stats->seen_through = (int64_t)h[CS_SEEN];
        stats->kept = cv.mask.kept, stats->transient = n - stats->kept;
    }
    return DMSA_OK;
}

int dmsa_dense_cloud_remove_transients(dmsa_dense_cloud* dc, int64_t* kept) {
    if (kept) *kept = 0;
    if (!dc) return DMSA_ERR_INVALID;
    return dense_remove_rows(dc, dc->carve.mask, "dense carve: no pass counts of the store as it stands (dmsa_dense_cloud_count_passes first)", "dense carve", kept);
}

}  // extern "C"
