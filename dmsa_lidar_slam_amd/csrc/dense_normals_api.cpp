// dense_normals_api.cpp — include/dmsa_dense_normals.h on top of dense_normals.hip: N1's checks, the launch sequence of the moments and the
// normals over the search grid of the store, and the file of the store with its normals.  The store, the grid, the checks of the radius and
// the file writer are shared with the other stages (dense_store.cpp, dense_cloud_obj.h).  The header text and N4 on the host:
// dense_normals_text.cpp.
#include "dense_cloud_obj.h"

#include "dense_normals.h"

namespace {

// N1
int check_preconditions(dmsa_dense_cloud* dc, const dmsa_dense_normals_config* cfg) {
    CHK(dense_radius_preconditions(dc, cfg->radius, "dense normals"));
    if (cfg->min_neighbours < 0) return fail(dc->ctx, DMSA_ERR_INVALID, "dense normals: min_neighbours must be >= 0");
    return DMSA_OK;
}

// N2-N3 for rows [first, first + count) into normals.moments
int run_moments(dmsa_dense_cloud* dc, const dmsa_dense_normals_config* cfg, int64_t first, int64_t count) {
    dmsa_ctx* ctx = dc->ctx;
    SearchGrid& grid = dc->shared.grid;
    CHK(grid.build(ctx, dc->store.g.as<float4>(), dc->store.n, dense_radius_edge(cfg->radius)));
    HIPCHK(dc->normals.moments.ensure((size_t)count * 80));
    const float scale = std::ldexp(1.0f, 20 - dense_radius_exponent(cfg->radius)), r2 = cfg->radius * cfg->radius;
    launch_neighbour_moments(grid.view(), r2, scale, first, count, dc->normals.moments.as<long long>(), ctx->stream);
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}

}  // namespace

extern "C" {

int dmsa_dense_cloud_neighbour_moments(dmsa_dense_cloud* dc, const dmsa_dense_normals_config* cfg, int64_t first, int64_t count, int64_t* moments) {
    if (!dc || !cfg || first < 0 || count < 0 || (count > 0 && !moments)) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(dense_row_range(dc, first, count, "dense normals"));
    if (count == 0) return DMSA_OK;
    CHK(set_device(ctx));
    CHK(run_moments(dc, cfg, first, count));
    HIPCHK(hipMemcpyAsync(moments, dc->normals.moments.p, (size_t)count * 80, hipMemcpyDeviceToHost, ctx->stream));
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
    DenseNormals& nr = dc->normals;
    nr.valid = false;
    const int64_t n = dc->store.n;
    CHK(run_moments(dc, cfg, 0, n));
    HIPCHK(nr.normal.ensure((size_t)n * 16));
    HIPCHK(nr.without.ensure(sizeof(unsigned long long)));
    HIPCHK(nr.h_without.ensure(sizeof(unsigned long long), nullptr));
    unsigned long long* without = nr.without.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(without, 0, 8, ctx->stream));
    launch_normals_from_moments(nr.moments.as<long long>(), dc->store.g.as<float4>(), dc->store.o.as<float4>(), 0, n, cfg->min_neighbours, nr.normal.as<float4>(), without,
                                ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(nr.h_without.p, without, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (normal_out) HIPCHK(hipMemcpyAsync(normal_out, nr.normal.p, (size_t)n * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    nr.moments.release();  // 80 bytes per row: not kept beside the result
    nr.valid = true;
    if (total) *total = n;
    if (without_normal) *without_normal = (int64_t)*nr.h_without.as<unsigned long long>();
    return DMSA_OK;
}

int dmsa_dense_cloud_save_pcd_normals(dmsa_dense_cloud* dc, const char* path, int64_t* points_out, int64_t* bytes_out) {
    if (points_out) *points_out = 0;
    if (bytes_out) *bytes_out = 0;
    if (!dc || !path) return DMSA_ERR_INVALID;
    if (!dc->normals.valid || dc->store.n < 1)
        return fail(dc->ctx, DMSA_ERR_INVALID, "dense normals: no normals since the last added scan (dmsa_dense_cloud_compute_normals first)");
    return dense_save_rows(dc, path, "dense normals", dc->point_floats() + 4, points_out, bytes_out);
}

}  // extern "C"
