// dense_compare_api.cpp — include/dmsa_dense_compare.h on top of dense_compare.hip: the reference cloud of an object (D0: the upload, the
// transform, the validity), D1's checks, the pair pass of a direction (both search grids cut with one edge, k_nearest_across, the sums: also
// what an iteration of dense_align_api.cpp runs), the launch sequence of a comparison (both directions, one host read, D5 on the host), of a
// classification (the flags, their scan into the stage's row mask), the removal by that mask (D6) and the file of D7.  Store, grid, mask and
// the shared checks: dense_store.cpp (dense_cloud_obj.h).  The defaults, D5 itself, the header and the reader of D8: dense_compare_text.cpp.
#include "dense_cloud_obj.h"

#include "dense_compare.h"

#include <cstring>
#include <vector>

namespace {

constexpr const char* kWhat = "dense compare";

int refuse(dmsa_dense_cloud* dc, const std::string& why) { return fail(dc->ctx, DMSA_ERR_INVALID, std::string(kWhat) + ": " + why); }

// D1, each stated once
int reference_ready(dmsa_dense_cloud* dc) {
    if (dc->compare.ref_rows < 1) return refuse(dc, "no reference cloud (dmsa_dense_cloud_set_reference first)");
    return dc->compare.ref_valid_rows < 1 ? refuse(dc, "the reference cloud has no valid row") : DMSA_OK;
}
int config_accepted(dmsa_dense_cloud* dc, const dmsa_dense_compare_config* cfg) {
    const char* why = dense_compare_config_refusal(cfg);
    return why ? refuse(dc, why) : DMSA_OK;
}
int check_preconditions(dmsa_dense_cloud* dc, const dmsa_dense_compare_config* cfg) {
    CHK(dense_reach_preconditions(dc, cfg->max_distance, "max_distance", kWhat));
    CHK(reference_ready(dc));
    CHK(config_accepted(dc, cfg));
    return dense_row_cap(dc, kWhat);
}
int reference_row_range(dmsa_dense_cloud* dc, int64_t first, int64_t count) {
    return first > dc->compare.ref_rows || count > dc->compare.ref_rows - first ? refuse(dc, "rows beyond the reference cloud") : DMSA_OK;
}

float scale_of(const dmsa_dense_compare_config* cfg) { return std::ldexp(1.0f, 18 - dense_radius_exponent(cfg->max_distance)); }

// the buffers of a call; both sums blocks zeroed on the stream
int begin_call(dmsa_dense_cloud* dc) {
    dmsa_ctx* ctx = dc->ctx;
    DenseCompare& cm = dc->compare;
    HIPCHK(cm.sums.ensure(2 * CM_COUNT * 8));
    HIPCHK(cm.h_sums.ensure(2 * CM_COUNT * 8 + 8, nullptr));
    HIPCHK(hipMemsetAsync(cm.sums.p, 0, 2 * CM_COUNT * 8, ctx->stream));
    return DMSA_OK;
}

// D2-D4 of one direction of a comparison: tolerance^2 is the `within` threshold, the direction's block of cm.sums takes the sums
int enqueue_direction(dmsa_dense_cloud* dc, const dmsa_dense_compare_config* cfg, int dir, int64_t first, int64_t count) {
    return dense_enqueue_pairs(dc, dir, first, count, cfg->max_distance, float_bits(cfg->tolerance * cfg->tolerance), dc->compare.sums.as<unsigned long long>() + dir * CM_COUNT);
}
void fill_header(dmsa_dense_cloud* dc, const dmsa_dense_compare_config* cfg, dmsa_dense_compare_stats* s) {
    const int e = dense_radius_exponent(cfg->max_distance);
    s->rows = dc->store.n, s->ref_rows = dc->compare.ref_rows, s->ref_invalid = dc->compare.ref_rows - dc->compare.ref_valid_rows;
    s->scale = (double)scale_of(cfg), s->bin_width_m = std::ldexp(1.0, e - 6);
}

int stage_call(dmsa_dense_cloud* dc, const dmsa_dense_compare_config* cfg, int dir, int64_t first, int64_t count, float* dist_out, int32_t* index_out) {
    if (!dc || !cfg || first < 0 || count < 0) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(dir == 0 ? dense_row_range(dc, first, count, kWhat) : reference_row_range(dc, first, count));
    if (count == 0) return DMSA_OK;
    CHK(set_device(ctx));
    CHK(begin_call(dc));
    CHK(enqueue_direction(dc, cfg, dir, first, count));
    DenseCompare& cm = dc->compare;
    if (dist_out) HIPCHK(hipMemcpyAsync(dist_out, cm.dist[dir].p, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (index_out) HIPCHK(hipMemcpyAsync(index_out, cm.index[dir].p, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (dir == 0 && first == 0 && count == dc->store.n) cm.dist_rows = count;
    return DMSA_OK;
}

}  // namespace

void dense_drop_reference(dmsa_dense_cloud* dc) {
    DenseCompare& cm = dc->compare;
    cm.ref_rows = 0, cm.ref_valid_rows = 0, cm.ref_grid.rows = 0, cm.dist_rows = -1, cm.mask.rows = -1;
}

int dense_reference_rows_accepted(dmsa_dense_cloud* dc, const float* xyz, int64_t n, int32_t stride_floats, int64_t least, const char* too_few, const char* what) {
    if (n < least || (n > 0 && !xyz)) return fail(dc->ctx, DMSA_ERR_INVALID, std::string(what) + ": " + too_few);
    if (n > 0 && stride_floats < 3) return fail(dc->ctx, DMSA_ERR_INVALID, std::string(what) + ": stride_floats must be at least 3");
    if (n > kMaxReference) return fail(dc->ctx, DMSA_ERR_INVALID, std::string(what) + ": more than 2^26 reference rows");
    return DMSA_OK;
}

int dense_upload_reference_rows(dmsa_dense_cloud* dc, const float* xyz, int64_t n, int32_t stride_floats, DevBuf* raw) {
    dmsa_ctx* ctx = dc->ctx;
    const size_t bytes = (size_t)n * (size_t)stride_floats * 4;
    HIPCHK(raw->ensure(bytes));
    HIPCHK(hipMemcpyAsync(raw->p, xyz, bytes, hipMemcpyHostToDevice, ctx->stream));
    return DMSA_OK;
}

int dense_enqueue_pairs(dmsa_dense_cloud* dc, int dir, int64_t first, int64_t count, float reach, uint32_t within_bits, unsigned long long* sums) {
    dmsa_ctx* ctx = dc->ctx;
    DenseCompare& cm = dc->compare;
    if (dir == 0) cm.dist_rows = -1;  // (the accuracy buffers are being rewritten)
    const bool pairs = cm.ref_valid_rows > 0;  // (a reference without a valid row has no grid and no pair: every query stays unmatched)
    SearchGrid& store_grid = dc->shared.grid;
    if (pairs) {
        const double edge = dense_radius_edge(reach);  // one edge for both grids: a key means the same cell in both
        CHK(store_grid.build(ctx, dc->store.g.as<float4>(), dc->store.n, edge));
        CHK(cm.ref_grid.build(ctx, cm.ref.as<float4>(), cm.ref_rows, edge, cm.ref_valid.as<uint8_t>(), cm.ref_valid_rows));
    }
    const size_t uc = (size_t)count;
    HIPCHK(cm.best[dir].ensure(uc * 8));
    HIPCHK(cm.dist[dir].ensure(uc * 4));
    HIPCHK(cm.index[dir].ensure(uc * 4));
    unsigned long long* best = cm.best[dir].as<unsigned long long>();
    HIPCHK(hipMemsetAsync(best, 0xFF, uc * 8, ctx->stream));  // kCompareNoMatch
    const float r2 = reach * reach;
    if (pairs && dir == 0) launch_nearest_across(store_grid.view(), cm.ref_grid.view(), r2, first, count, best, ctx->stream);
    if (pairs && dir == 1) launch_nearest_across(cm.ref_grid.view(), store_grid.view(), r2, first, count, best, ctx->stream);
    launch_compare_quantise_sum(best, dir == 0 ? nullptr : cm.ref_valid.as<uint8_t>() + first, count, std::ldexp(1.0f, 18 - dense_radius_exponent(reach)), within_bits,
                                cm.dist[dir].as<float>(), cm.index[dir].as<int32_t>(), sums, ctx->stream);
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}

int dense_fill_direction(dmsa_dense_cloud* dc, const unsigned long long* h, int64_t queries, double scale, const char* what, dmsa_dense_compare_direction* d) {
    *d = dmsa_dense_compare_direction{};
    d->queries = queries, d->matched = (int64_t)h[CM_MATCHED], d->unmatched = (int64_t)h[CM_UNMATCHED], d->within = (int64_t)h[CM_WITHIN];
    d->s1 = (int64_t)h[CM_S1], d->s2 = (int64_t)h[CM_S2];
    for (int b = 0; b < DMSA_COMPARE_BINS; ++b) d->histogram[b] = (int64_t)h[CM_BINS + b];
    if (dmsa_dense_compare_summary(d->matched, d->s1, d->s2, d->within, queries, scale, &d->mean_m, &d->rms_m, &d->fraction_within) != DMSA_OK)
        return fail(dc->ctx, DMSA_ERR_INVALID, std::string(what) + ": the sums of D4 left their range");  // (never: D1)
    return DMSA_OK;
}

int dense_reference_from_device_rows(dmsa_dense_cloud* dc, const float* d_raw, int64_t n, int32_t stride_floats, const double* T) {
    dmsa_ctx* ctx = dc->ctx;
    DenseCompare& cm = dc->compare;
    dense_drop_reference(dc);
    dmsa::RefTransform t{};
    if (T)
        for (int i = 0; i < 12; ++i) t.c[i] = (float)T[i];
    const size_t un = (size_t)n;
    HIPCHK(cm.ref.ensure(un * 16));
    HIPCHK(cm.ref_valid.ensure(un));
    HIPCHK(cm.sums.ensure(2 * CM_COUNT * 8));
    HIPCHK(cm.h_sums.ensure(2 * CM_COUNT * 8 + 8, nullptr));
    unsigned long long* invalid = cm.sums.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(invalid, 0, 8, ctx->stream));
    launch_reference_transform(d_raw, n, stride_floats, T != nullptr, t, dc->cfg.voxel_size, cm.ref.as<float4>(), cm.ref_valid.as<uint8_t>(), invalid, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cm.h_sums.p, invalid, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    cm.ref_rows = n, cm.ref_valid_rows = n - (int64_t)*cm.h_sums.as<unsigned long long>();
    return DMSA_OK;
}

extern "C" {

int dmsa_dense_cloud_set_reference(dmsa_dense_cloud* dc, const float* xyz, int64_t n, int32_t stride_floats, const double* T) {
    if (!dc) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(dense_reference_rows_accepted(dc, xyz, n, stride_floats, 0, "a reference of a negative number of rows, or rows without a pointer", kWhat));
    if (n > 0 && !(dc->cfg.voxel_size > 0.0f)) return refuse(dc, "voxel_size must be > 0 (D0 bounds the reference by the voxel grid)");
    if (T)
        for (int i = 0; i < 12; ++i)
            if (!std::isfinite(T[i])) return refuse(dc, "the transform is not finite");
    // whatever fails from here on leaves no reference; the results against the old one are stale either way
    dense_drop_reference(dc);
    if (n == 0) return DMSA_OK;
    CHK(set_device(ctx));
    DevBuf raw;  // the caller's rows as they came, released with this call
    CHK(dense_upload_reference_rows(dc, xyz, n, stride_floats, &raw));
    const int rc = dense_reference_from_device_rows(dc, raw.as<float>(), n, stride_floats, T);
    if (rc != DMSA_OK) (void)hipStreamSynchronize(ctx->stream);  // (the copy reads the caller's rows and writes `raw`)
    return rc;
}

int dmsa_dense_cloud_reference(dmsa_dense_cloud* dc, int64_t first, int64_t count, float* xyz_out, uint8_t* valid_out, int64_t* total_out) {
    if (total_out) *total_out = 0;
    if (!dc || first < 0 || count < 0) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    DenseCompare& cm = dc->compare;
    if (total_out) *total_out = cm.ref_rows;
    CHK(reference_row_range(dc, first, count));
    if (count == 0) return DMSA_OK;
    CHK(set_device(ctx));
    std::vector<float> rows;
    if (xyz_out) {
        rows.resize((size_t)count * 4);
        HIPCHK(hipMemcpyAsync(rows.data(), cm.ref.as<float4>() + first, (size_t)count * 16, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (valid_out) HIPCHK(hipMemcpyAsync(valid_out, cm.ref_valid.as<uint8_t>() + first, (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (xyz_out)
        for (int64_t i = 0; i < count; ++i) std::memcpy(xyz_out + 3 * i, rows.data() + 4 * i, 12);
    return DMSA_OK;
}

int dmsa_dense_cloud_nearest_in_reference(dmsa_dense_cloud* dc, const dmsa_dense_compare_config* cfg, int64_t first, int64_t count, float* dist_out, int32_t* index_out) {
    return stage_call(dc, cfg, 0, first, count, dist_out, index_out);
}
int dmsa_dense_cloud_nearest_in_store(dmsa_dense_cloud* dc, const dmsa_dense_compare_config* cfg, int64_t first, int64_t count, float* dist_out, int32_t* index_out) {
    return stage_call(dc, cfg, 1, first, count, dist_out, index_out);
}

int dmsa_dense_cloud_compare(dmsa_dense_cloud* dc, const dmsa_dense_compare_config* cfg, dmsa_dense_compare_stats* stats) {
    if (stats) *stats = dmsa_dense_compare_stats{};
    if (!dc || !cfg) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(set_device(ctx));
    DenseCompare& cm = dc->compare;
    const int64_t n = dc->store.n;
    CHK(begin_call(dc));
    CHK(enqueue_direction(dc, cfg, 0, 0, n));
    CHK(enqueue_direction(dc, cfg, 1, 0, cm.ref_rows));
    unsigned long long* h = cm.h_sums.as<unsigned long long>();
    HIPCHK(hipMemcpyAsync(h, cm.sums.p, 2 * CM_COUNT * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // the one host read
    cm.dist_rows = n;
    dmsa_dense_compare_stats s{};
    fill_header(dc, cfg, &s);
    CHK(dense_fill_direction(dc, h, n, s.scale, kWhat, &s.accuracy));
    CHK(dense_fill_direction(dc, h + CM_COUNT, cm.ref_valid_rows, s.scale, kWhat, &s.completeness));
    s.precision = s.accuracy.fraction_within, s.recall = s.completeness.fraction_within;
    const double pr = s.precision + s.recall;
    s.f_score = pr > 0.0 ? 2.0 * s.precision * s.recall / pr : 0.0;
    if (stats) *stats = s;
    return DMSA_OK;
}

int dmsa_dense_cloud_classify_by_reference(dmsa_dense_cloud* dc, const dmsa_dense_compare_config* cfg, uint8_t* keep_out, dmsa_dense_compare_stats* stats) {
    if (stats) *stats = dmsa_dense_compare_stats{};
    if (!dc || !cfg) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    CHK(check_preconditions(dc, cfg));
    CHK(set_device(ctx));
    DenseCompare& cm = dc->compare;
    const int64_t n = dc->store.n;
    const size_t un = (size_t)n;
    HIPCHK(cm.mask.begin(n));
    CHK(begin_call(dc));
    CHK(enqueue_direction(dc, cfg, 0, 0, n));
    HIPCHK(cm.flag8.ensure(un));
    unsigned long long* sums = cm.sums.as<unsigned long long>();
    unsigned long long* h = cm.h_sums.as<unsigned long long>();
    launch_compare_flags(cm.best[0].as<unsigned long long>(), n, float_bits(cfg->tolerance * cfg->tolerance), cfg->keep == DMSA_COMPARE_KEEP_NEAR,
                         cm.mask.keep.as<int32_t>(), cm.flag8.as<uint8_t>(), sums, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(cm.mask.enqueue_scan(n, dc->shared.scan_tmp, ctx->stream));
    HIPCHK(hipMemcpyAsync(h, sums, 2 * CM_COUNT * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(cm.mask.enqueue_count(n, cm.h_sums.as<int32_t>() + 4 * CM_COUNT, ctx->stream));
    if (keep_out) HIPCHK(hipMemcpyAsync(keep_out, cm.flag8.p, un, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // the one host read
    cm.mask.commit(n);
    cm.dist_rows = n;
    dmsa_dense_compare_stats s{};
    fill_header(dc, cfg, &s);
    CHK(dense_fill_direction(dc, h, n, s.scale, kWhat, &s.accuracy));
    s.precision = s.accuracy.fraction_within;
    s.kept = cm.mask.kept;
    if (s.kept != (int64_t)h[CM_KEPT]) return cm.mask.rows = -1, fail(ctx, DMSA_ERR_HIP, "dense compare: the scan of the flags and their count disagree");  // (never)
    if (stats) *stats = s;
    return DMSA_OK;
}

int dmsa_dense_cloud_remove_by_reference(dmsa_dense_cloud* dc, int64_t* kept) {
    if (kept) *kept = 0;
    if (!dc) return DMSA_ERR_INVALID;
    return dense_remove_rows(dc, dc->compare.mask, "dense compare: no classification of the store as it stands (dmsa_dense_cloud_classify_by_reference first)",
                             kWhat, kept);
}

int dmsa_dense_cloud_save_pcd_distance(dmsa_dense_cloud* dc, const char* path, int64_t* points_out, int64_t* bytes_out) {
    if (points_out) *points_out = 0;
    if (bytes_out) *bytes_out = 0;
    if (!dc || !path) return DMSA_ERR_INVALID;
    CHK(dense_retention_on(dc, kWhat));
    if (dc->store.n < 1) return refuse(dc, "no retained point to write");
    if (dc->compare.ref_rows < 1 || !dc->compare.distances_valid_for(dc->store))
        return refuse(dc, "no distances of the store as it stands against the reference as it stands (dmsa_dense_cloud_compare or classify_by_reference first)");
    return dense_save_rows(dc, path, kWhat, dc->point_floats(), points_out, bytes_out, RowWord::distance);
}

}  // extern "C"
