// dense_outliers_api.cpp — include/dmsa_dense_outliers.h on top of dense_outliers.hip: O1's checks, the launch sequence of a classification
// (the grid of dense_normals_api.cpp, k_knn_mean_distance, the sums, one host read, O5 on the host, the flags and their scan), the removal (O6: dense_compact_store
// of dense_cloud_obj.h) and the x y z file of the store.  O5 itself and the defaults: dense_outliers_text.cpp.
#include "dense_cloud_obj.h"

#include "dense_outliers.h"

namespace {

constexpr int64_t kMaxOutlierRows = (int64_t)1 << 26;  // O1

// O1
int check_preconditions(dmsa_dense_cloud* dc, const dmsa_dense_outlier_config* cfg) {
    dmsa_ctx* ctx = dc->ctx;
    CHK(dense_radius_preconditions(dc, cfg->radius, "dense outliers"));
    if (cfg->k < 1 || cfg->k > kOutlierMaxK) return fail(ctx, DMSA_ERR_INVALID, "dense outliers: k must lie in [1, 16]");
    if (!std::isfinite(cfg->stddev_mul) || cfg->stddev_mul < 0.0f) return fail(ctx, DMSA_ERR_INVALID, "dense outliers: stddev_mul must be finite and >= 0");
    if (dc->ret_n > kMaxOutlierRows) return fail(ctx, DMSA_ERR_INVALID, "dense outliers: more than 2^26 retained rows");
    return DMSA_OK;
}

// O2-O3 for rows [first, first + count) into st->knn_mean
int run_knn(dmsa_dense_cloud* dc, DenseNormalsState* st, const dmsa_dense_outlier_config* cfg, int64_t first, int64_t count) {
    dmsa_ctx* ctx = dc->ctx;
    CHK(dense_normals_grid(dc, st, dense_radius_edge(cfg->radius)));
    HIPCHK(st->knn_mean.ensure((size_t)count * 4));
    launch_knn_mean_distance(st->pts.as<float4>(), st->idx_s.as<uint32_t>(), st->key_s.as<unsigned long long>(), dc->ret_n, st->table.as<DenseCellEntry>(), st->mask,
                             cfg->radius * cfg->radius, cfg->k, first, count, st->knn_mean.as<float>(), ctx->stream);
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}

}  // namespace

extern "C" {

int dmsa_dense_cloud_knn_mean_distance(dmsa_dense_cloud* dc, const dmsa_dense_outlier_config* cfg, int64_t first, int64_t count, float* mean_out) {
    if (!dc || !cfg || first < 0 || count < 0 || (count > 0 && !mean_out)) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    if (first > dc->ret_n || count > dc->ret_n - first) return fail(ctx, DMSA_ERR_INVALID, "dense outliers: rows beyond the retained store");
    if (count == 0) return DMSA_OK;
    CHK(set_device(ctx));
    DenseNormalsState* st = nullptr;
    CHK(dense_normals_state(dc, &st));
    CHK(run_knn(dc, st, cfg, first, count));
    HIPCHK(hipMemcpyAsync(mean_out, st->knn_mean.p, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DMSA_OK;
}

int dmsa_dense_cloud_classify_outliers(dmsa_dense_cloud* dc, const dmsa_dense_outlier_config* cfg, uint8_t* inlier_out, dmsa_dense_outlier_stats* stats) {
    if (stats) *stats = dmsa_dense_outlier_stats{};
    if (!dc || !cfg) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(set_device(ctx));
    DenseNormalsState* st = nullptr;
    CHK(dense_normals_state(dc, &st));
    st->flags_n = -1;
    const int64_t n = dc->ret_n;
    const size_t un = (size_t)n;
    CHK(run_knn(dc, st, cfg, 0, n));
    HIPCHK(st->knn_q.ensure(un * 4));
    HIPCHK(st->keep.ensure((un + 1) * 4));
    HIPCHK(st->keep_scan.ensure((un + 1) * 4));
    HIPCHK(st->flag8.ensure(un));
    HIPCHK(st->scan_tmp.ensure(scan_temp_bytes(un + 1)));
    HIPCHK(st->sums.ensure(OS_COUNT * 8));
    HIPCHK(st->h_sums.ensure(OS_COUNT * 8 + 8, nullptr));
    int e = 0;
    (void)std::frexp(cfg->radius, &e);
    const float scale = std::ldexp(1.0f, 18 - e);
    unsigned long long* sums = st->sums.as<unsigned long long>();
    unsigned long long* h = st->h_sums.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(sums, 0, OS_COUNT * 8, ctx->stream));
    launch_outlier_quantise_sum(st->knn_mean.as<float>(), n, scale, st->knn_q.as<int32_t>(), sums, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, sums, OS_COUNT * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // the one host read between the sums and the flags
    dmsa_dense_outlier_stats s{};
    s.rows = n, s.isolated = (int64_t)h[OS_ISOLATED], s.n_s = (int64_t)h[OS_N], s.s1 = (int64_t)h[OS_S1], s.s2 = (int64_t)h[OS_S2];
    double mean = 0.0, sd = 0.0, threshold = 0.0;
    if (dmsa_dense_outlier_threshold(s.n_s, s.s1, s.s2, cfg->stddev_mul, &mean, &sd, &threshold) != DMSA_OK)
        return fail(ctx, DMSA_ERR_INVALID, "dense outliers: the sums of O4 left their range");  // (never: O1)
    launch_outlier_flags(st->knn_q.as<int32_t>(), n, threshold, st->keep.as<int32_t>(), st->flag8.as<uint8_t>(), ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(exclusive_scan_i32(st->scan_tmp.p, st->scan_tmp.cap, st->keep.as<int32_t>(), st->keep_scan.as<int32_t>(), un + 1, ctx->stream));
    int32_t* h_inliers = reinterpret_cast<int32_t*>(h + OS_COUNT);
    HIPCHK(hipMemcpyAsync(h_inliers, st->keep_scan.as<int32_t>() + n, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (inlier_out) HIPCHK(hipMemcpyAsync(inlier_out, st->flag8.p, un, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.inliers = *h_inliers, s.above_threshold = n - s.isolated - s.inliers;
    s.mean_m = mean / (double)scale, s.stddev_m = sd / (double)scale, s.threshold_m = threshold / (double)scale;
    st->flags_n = n;
    if (stats) *stats = s;
    return DMSA_OK;
}

int dmsa_dense_cloud_remove_outliers(dmsa_dense_cloud* dc, int64_t* kept) {
    if (kept) *kept = 0;
    if (!dc) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    DenseNormalsState* st = dc->nrm;
    if (kept) *kept = dc->ret_n;
    if (!dc->retain || !st || st->flags_n < 0 || st->flags_n != dc->ret_n)
        return fail(ctx, DMSA_ERR_INVALID, "dense outliers: no classification of the store as it stands (dmsa_dense_cloud_classify_outliers first)");
    CHK(set_device(ctx));
    const int64_t m = *reinterpret_cast<int32_t*>(st->h_sums.as<unsigned long long>() + OS_COUNT);
    CHK(dense_compact_store(dc, st->keep.as<int32_t>(), st->keep_scan.as<int32_t>(), m, "dense outliers"));
    if (kept) *kept = m;
    return DMSA_OK;
}

int dmsa_dense_cloud_save_pcd_retained(dmsa_dense_cloud* dc, const char* path, int64_t* points_out, int64_t* bytes_out) {
    if (points_out) *points_out = 0;
    if (bytes_out) *bytes_out = 0;
    if (!dc || !path) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    if (!dc->retain) return fail(ctx, DMSA_ERR_INVALID, "dense outliers: retention is off (dmsa_dense_cloud_retain before the first scan)");
    if (dc->ret_n < 1) return fail(ctx, DMSA_ERR_INVALID, "dense outliers: no retained point to write");
    CHK(set_device(ctx));
    DenseNormalsState* st = nullptr;
    CHK(dense_normals_state(dc, &st));
    return dense_save_rows(dc, st, path, "dense outliers", 3, points_out, bytes_out);
}

}  // extern "C"
