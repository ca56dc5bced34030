// dense_outliers_api.cpp — include/dmsa_dense_outliers.h on top of dense_outliers.hip: O1's checks, the launch sequence of a classification
// (the search grid of the store, k_knn_mean_distance, the sums, one host read, O5 on the host, the flags and their scan into the stage's row
// mask), the removal by that mask (O6) and the x y z file of the store.  Store, grid, mask and the shared checks: dense_store.cpp
// (dense_cloud_obj.h).  O5 itself and the defaults: dense_outliers_text.cpp.
#include "dense_cloud_obj.h"

#include "dense_outliers.h"

namespace {

// O1
int check_preconditions(dmsa_dense_cloud* dc, const dmsa_dense_outlier_config* cfg) {
    dmsa_ctx* ctx = dc->ctx;
    CHK(dense_radius_preconditions(dc, cfg->radius, "dense outliers"));
    if (cfg->k < 1 || cfg->k > kOutlierMaxK) return fail(ctx, DMSA_ERR_INVALID, "dense outliers: k must lie in [1, 16]");
    if (!std::isfinite(cfg->stddev_mul) || cfg->stddev_mul < 0.0f) return fail(ctx, DMSA_ERR_INVALID, "dense outliers: stddev_mul must be finite and >= 0");
    return dense_row_cap(dc, "dense outliers");
}

// O2-O3 for rows [first, first + count) into outliers.knn_mean
int run_knn(dmsa_dense_cloud* dc, const dmsa_dense_outlier_config* cfg, int64_t first, int64_t count) {
    dmsa_ctx* ctx = dc->ctx;
    SearchGrid& grid = dc->shared.grid;
    CHK(grid.build(ctx, dc->store.g.as<float4>(), dc->store.n, dense_radius_edge(cfg->radius)));
    HIPCHK(dc->outliers.knn_mean.ensure((size_t)count * 4));
    launch_knn_mean_distance(grid.view(), cfg->radius * cfg->radius, cfg->k, first, count, dc->outliers.knn_mean.as<float>(), ctx->stream);
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}

}  // namespace

extern "C" {

int dmsa_dense_cloud_knn_mean_distance(dmsa_dense_cloud* dc, const dmsa_dense_outlier_config* cfg, int64_t first, int64_t count, float* mean_out) {
    if (!dc || !cfg || first < 0 || count < 0 || (count > 0 && !mean_out)) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(dense_row_range(dc, first, count, "dense outliers"));
    if (count == 0) return DMSA_OK;
    CHK(set_device(ctx));
    CHK(run_knn(dc, cfg, first, count));
    HIPCHK(hipMemcpyAsync(mean_out, dc->outliers.knn_mean.p, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

int dmsa_dense_cloud_classify_outliers(dmsa_dense_cloud* dc, const dmsa_dense_outlier_config* cfg, uint8_t* inlier_out, dmsa_dense_outlier_stats* stats) {
    if (stats) *stats = dmsa_dense_outlier_stats{};
    if (!dc || !cfg) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(set_device(ctx));
    DenseOutliers& ol = dc->outliers;
    const int64_t n = dc->store.n;
    const size_t un = (size_t)n;
    HIPCHK(ol.mask.begin(n));
    CHK(run_knn(dc, cfg, 0, n));
    HIPCHK(ol.knn_q.ensure(un * 4));
    HIPCHK(ol.flag8.ensure(un));
    HIPCHK(ol.sums.ensure(OS_COUNT * 8));
    HIPCHK(ol.h_sums.ensure(OS_COUNT * 8 + 8, nullptr));
    const float scale = std::ldexp(1.0f, 18 - dense_radius_exponent(cfg->radius));
    unsigned long long* sums = ol.sums.as<unsigned long long>();
    unsigned long long* h = ol.h_sums.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(sums, 0, OS_COUNT * 8, ctx->stream));
    launch_outlier_quantise_sum(ol.knn_mean.as<float>(), n, scale, ol.knn_q.as<int32_t>(), sums, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, sums, OS_COUNT * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // the one host read between the sums and the flags
    dmsa_dense_outlier_stats s{};
    s.rows = n, s.isolated = (int64_t)h[OS_ISOLATED], s.n_s = (int64_t)h[OS_N], s.s1 = (int64_t)h[OS_S1], s.s2 = (int64_t)h[OS_S2];
    double mean = 0.0, sd = 0.0, threshold = 0.0;
    if (dmsa_dense_outlier_threshold(s.n_s, s.s1, s.s2, cfg->stddev_mul, &mean, &sd, &threshold) != DMSA_OK)
        return fail(ctx, DMSA_ERR_INVALID, "dense outliers: the sums of O4 left their range");  // (never: O1)
    launch_outlier_flags(ol.knn_q.as<int32_t>(), n, threshold, ol.mask.keep.as<int32_t>(), ol.flag8.as<uint8_t>(), ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(ol.mask.enqueue_scan(n, dc->shared.scan_tmp, ctx->stream));
    HIPCHK(ol.mask.enqueue_count(n, ol.h_sums.as<int32_t>() + 2 * OS_COUNT, ctx->stream));
    if (inlier_out) HIPCHK(hipMemcpyAsync(inlier_out, ol.flag8.p, un, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ol.mask.commit(n);
    s.inliers = ol.mask.kept, s.above_threshold = n - s.isolated - s.inliers;
    s.mean_m = mean / (double)scale, s.stddev_m = sd / (double)scale, s.threshold_m = threshold / (double)scale;
    if (stats) *stats = s;
    return DMSA_OK;
}

int dmsa_dense_cloud_remove_outliers(dmsa_dense_cloud* dc, int64_t* kept) {
    if (kept) *kept = 0;
    if (!dc) return DMSA_ERR_INVALID;
    return dense_remove_rows(dc, dc->outliers.mask, "dense outliers: no classification of the store as it stands (dmsa_dense_cloud_classify_outliers first)",
                             "dense outliers", kept);
}

int dmsa_dense_cloud_save_pcd_retained(dmsa_dense_cloud* dc, const char* path, int64_t* points_out, int64_t* bytes_out) {
    if (points_out) *points_out = 0;
    if (bytes_out) *bytes_out = 0;
    if (!dc || !path) return DMSA_ERR_INVALID;
    CHK(dense_retention_on(dc, "dense outliers"));
    if (dc->store.n < 1) return fail(dc->ctx, DMSA_ERR_INVALID, "dense outliers: no retained point to write");
    return dense_save_rows(dc, path, "dense outliers", dc->point_floats(), points_out, bytes_out);
}

}  // extern "C"
