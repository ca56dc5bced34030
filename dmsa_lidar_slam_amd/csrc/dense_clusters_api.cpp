// dense_clusters_api.cpp — include/dmsa_dense_clusters.h on top of dense_clusters.hip: C1's checks, the launch sequence of a labelling (the
// search grid of the store, k_cluster_link, the flattening, the smallest row and the size per root, labels in store-row terms), of a
// classification (the flags, their scan into the stage's row mask, one host read of the sums and the give-up word), the removal by that
// mask (C6) and the file of C7.  Store, grid, mask and the shared checks: dense_store.cpp (dense_cloud_obj.h).  The defaults, the checks
// of the two sizes and the header: dense_clusters_text.cpp.
#include "dense_cloud_obj.h"

#include "dense_clusters.h"

namespace {

// C1
int check_preconditions(dmsa_dense_cloud* dc, const dmsa_dense_cluster_config* cfg) {
    CHK(dense_radius_preconditions(dc, cfg->radius, "dense clusters"));
    const char* why = dense_cluster_config_refusal(cfg);
    if (why) return fail(dc->ctx, DMSA_ERR_INVALID, std::string("dense clusters: ") + why);
    return dense_row_cap(dc, "dense clusters");
}

// the buffers of a call; the sums block zeroed on the stream
int begin_call(dmsa_dense_cloud* dc) {
    dmsa_ctx* ctx = dc->ctx;
    DenseClusters& cl = dc->clusters;
    HIPCHK(cl.sums.ensure(CL_COUNT * 8));
    HIPCHK(cl.h_sums.ensure(CL_COUNT * 8 + 8, nullptr));
    HIPCHK(hipMemsetAsync(cl.sums.p, 0, CL_COUNT * 8, ctx->stream));
    return DMSA_OK;
}

// C2-C3 enqueued: clusters.label / clusters.size of all rows at cfg->radius.  Labels of the store as it stands at the same radius are kept.
// The caller reads the sums block, synchronises and calls end_labels.
int enqueue_labels(dmsa_dense_cloud* dc, const dmsa_dense_cluster_config* cfg) {
    dmsa_ctx* ctx = dc->ctx;
    DenseClusters& cl = dc->clusters;
    if (cl.labels_valid_for(dc->store) && cl.label_radius == cfg->radius) return DMSA_OK;
    cl.label_rows = -1;
    SearchGrid& grid = dc->shared.grid;
    const int64_t n = dc->store.n;
    const size_t un = (size_t)n;
    CHK(grid.build(ctx, dc->store.g.as<float4>(), dc->store.n, dense_radius_edge(cfg->radius)));
    for (DevBuf* b : {&cl.parent, &cl.root, &cl.min_row, &cl.count, &cl.label, &cl.size}) HIPCHK(b->ensure(un * 4));
    uint32_t* parent = cl.parent.as<uint32_t>();
    uint32_t* root = cl.root.as<uint32_t>();
    unsigned long long* sums = cl.sums.as<unsigned long long>();
    launch_cluster_init(n, parent, cl.min_row.as<int32_t>(), cl.count.as<int32_t>(), ctx->stream);
    launch_cluster_link(grid.view(), cfg->radius * cfg->radius, parent, sums, ctx->stream);
    launch_cluster_flatten(grid.view(), parent, root, cl.min_row.as<int32_t>(), sums, ctx->stream);
    launch_cluster_sizes(n, root, cl.count.as<int32_t>(), ctx->stream);
    launch_cluster_rows(grid.view(), root, cl.min_row.as<int32_t>(), cl.count.as<int32_t>(), cl.label.as<int32_t>(), cl.size.as<int32_t>(), ctx->stream);
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}

// after the call's synchronisation: the give-up word of the sums block as read back
int end_labels(dmsa_dense_cloud* dc, const dmsa_dense_cluster_config* cfg) {
    DenseClusters& cl = dc->clusters;
    const unsigned long long gave_up = cl.h_sums.as<unsigned long long>()[CL_GAVE_UP];
    if (gave_up != 0ull) {
        cl.label_rows = -1;
        return fail(dc->ctx, DMSA_ERR_HIP,
                    std::string("dense clusters: the union-find gave up in ") + ((gave_up & kClusterGaveUpFind) ? "the walk to a root (d_find)" : "the hook's retry loop (d_unite)") +
                        " after as many rounds as there are rows");
    }
    cl.label_rows = dc->store.n, cl.label_radius = cfg->radius;
    return DMSA_OK;
}

}  // namespace

extern "C" {

int dmsa_dense_cloud_cluster_labels(dmsa_dense_cloud* dc, const dmsa_dense_cluster_config* cfg, int32_t* label_out, int32_t* size_out) {
    if (!dc || !cfg) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(set_device(ctx));
    DenseClusters& cl = dc->clusters;
    const size_t un = (size_t)dc->store.n;
    CHK(begin_call(dc));
    CHK(enqueue_labels(dc, cfg));
    HIPCHK(hipMemcpyAsync(cl.h_sums.p, cl.sums.p, CL_COUNT * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (label_out) HIPCHK(hipMemcpyAsync(label_out, cl.label.p, un * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (size_out) HIPCHK(hipMemcpyAsync(size_out, cl.size.p, un * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return end_labels(dc, cfg);
}

int dmsa_dense_cloud_classify_clusters(dmsa_dense_cloud* dc, const dmsa_dense_cluster_config* cfg, uint8_t* keep_out, dmsa_dense_cluster_stats* stats) {
    if (stats) *stats = dmsa_dense_cluster_stats{};
    if (!dc || !cfg) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(set_device(ctx));
    DenseClusters& cl = dc->clusters;
    const int64_t n = dc->store.n;
    const size_t un = (size_t)n;
    HIPCHK(cl.mask.begin(n));
    CHK(begin_call(dc));
    CHK(enqueue_labels(dc, cfg));
    HIPCHK(cl.flag8.ensure(un));
    unsigned long long* sums = cl.sums.as<unsigned long long>();
    unsigned long long* h = cl.h_sums.as<unsigned long long>();
    launch_cluster_flags(cl.label.as<int32_t>(), cl.size.as<int32_t>(), n, cfg->min_size, cfg->max_size, cl.mask.keep.as<int32_t>(), cl.flag8.as<uint8_t>(), sums, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(cl.mask.enqueue_scan(n, dc->shared.scan_tmp, ctx->stream));
    HIPCHK(hipMemcpyAsync(h, sums, CL_COUNT * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(cl.mask.enqueue_count(n, cl.h_sums.as<int32_t>() + 2 * CL_COUNT, ctx->stream));
    if (keep_out) HIPCHK(hipMemcpyAsync(keep_out, cl.flag8.p, un, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // the one host read
    CHK(end_labels(dc, cfg));
    cl.mask.commit(n);
    if (stats) {
        stats->rows = n, stats->clusters = (int64_t)h[CL_CLUSTERS], stats->largest = (int64_t)h[CL_LARGEST];
        stats->kept_rows = (int64_t)h[CL_KEPT_ROWS], stats->kept_clusters = (int64_t)h[CL_KEPT_CLUSTERS];
        stats->small_rows = (int64_t)h[CL_SMALL], stats->large_rows = (int64_t)h[CL_LARGE];
    }
    return DMSA_OK;
}

int dmsa_dense_cloud_remove_clusters(dmsa_dense_cloud* dc, int64_t* kept) {
    if (kept) *kept = 0;
    if (!dc) return DMSA_ERR_INVALID;
    return dense_remove_rows(dc, dc->clusters.mask, "dense clusters: no classification of the store as it stands (dmsa_dense_cloud_classify_clusters first)",
                             "dense clusters", kept);
}

int dmsa_dense_cloud_save_pcd_labels(dmsa_dense_cloud* dc, const char* path, int64_t* points_out, int64_t* bytes_out) {
    if (points_out) *points_out = 0;
    if (bytes_out) *bytes_out = 0;
    if (!dc || !path) return DMSA_ERR_INVALID;
    CHK(dense_retention_on(dc, "dense clusters"));
    if (dc->store.n < 1) return fail(dc->ctx, DMSA_ERR_INVALID, "dense clusters: no retained point to write");
    if (!dc->clusters.labels_valid_for(dc->store))
        return fail(dc->ctx, DMSA_ERR_INVALID, "dense clusters: no labels of the store as it stands (dmsa_dense_cloud_cluster_labels or classify_clusters first)");
    return dense_save_rows(dc, path, "dense clusters", dc->point_floats(), points_out, bytes_out, RowWord::label);
}

}  // extern "C"
