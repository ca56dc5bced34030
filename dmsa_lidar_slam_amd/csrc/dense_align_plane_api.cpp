// dense_align_plane_api.cpp — include/dmsa_dense_align_plane.h on top of dense_align_plane.hip and the kernels of dense_compare.hip: P0's
// checks, the launch sequence of one iteration's sums (dense_align_api.cpp's, with the store's normals and k_align_plane_sums in the place
// of k_align_pair_sums: both search grids cut with one edge, k_nearest_across in the completeness direction, D4's sums, P2's sums, one copy
// back through slot 1 of the stage's CopyBack), and the loop of P1-P9 on the context's stream: per iteration the reference transformed from
// the raw rows (dense_compare_api.cpp: D0's own path), the sums, then on the host the step (dense_align_plane_solve.cpp), A5's composition
// and P7's stopping rules.
#include "dense_cloud_obj.h"

#include "dense_align_plane.h"

#include <cstring>

namespace {

constexpr int64_t kMaxReference = (int64_t)1 << 26;  // D0
constexpr const char* kWhat = "dense align plane";
constexpr size_t kSumWords = (size_t)dmsa::kAlignPlaneSums + CM_COUNT;  // P2's 64 words, then D4's block of all matched pairs
constexpr int kSlot = 1;  // of DenseAlign::back; slot 0 is the point-to-point call's

int refuse(dmsa_dense_cloud* dc, const std::string& why) { return fail(dc->ctx, DMSA_ERR_INVALID, std::string(kWhat) + ": " + why); }

void drop_reference(dmsa_dense_cloud* dc) {
    DenseCompare& cm = dc->compare;
    cm.ref_rows = 0, cm.ref_valid_rows = 0, cm.ref_grid.rows = 0, cm.dist_rows = -1, cm.mask.rows = -1;
}

uint32_t float_bits(float v) {
    uint32_t b;
    return std::memcpy(&b, &v, 4), b;
}

// D1 of max_distance and of the store, P0 of the normals
int check_store(dmsa_dense_cloud* dc, float max_distance) {
    CHK(dense_reach_preconditions(dc, max_distance, "max_distance", kWhat));
    CHK(dense_row_cap(dc, kWhat));
    if (!dc->normals.valid || dc->normals.normal.cap < (size_t)dc->store.n * 16)
        return refuse(dc, "no normals of the store as it stands (dmsa_dense_cloud_compute_normals first)");
    return DMSA_OK;
}

// P2 and D4 of the reference as it stands against the store as it stands, waited for: *words = kSumWords words the host may read until the
// next call of this stage
int plane_sums(dmsa_dense_cloud* dc, float max_distance, const unsigned long long** words) {
    dmsa_ctx* ctx = dc->ctx;
    DenseCompare& cm = dc->compare;
    DenseAlign& al = dc->align;
    if (!al.created) {
        HIPCHK(al.back.create());
        al.created = true;
    }
    HIPCHK(al.back.reserve(kSlot, kSumWords * 8, kSumWords * 8));
    const size_t un = (size_t)cm.ref_rows;
    HIPCHK(cm.best[1].ensure(un * 8));
    HIPCHK(cm.dist[1].ensure(un * 4));
    HIPCHK(cm.index[1].ensure(un * 4));
    unsigned long long* best = cm.best[1].as<unsigned long long>();
    unsigned long long* sums = al.back.dev[kSlot].as<unsigned long long>();
    if (cm.ref_valid_rows > 0) {  // (a reference without a valid row has no grid and no pair: every word stays 0)
        const double edge = dense_radius_edge(max_distance);  // one edge for both grids: a key means the same cell in both
        CHK(dc->shared.grid.build(ctx, dc->store.g.as<float4>(), dc->store.n, edge));
        CHK(cm.ref_grid.build(ctx, cm.ref.as<float4>(), cm.ref_rows, edge, cm.ref_valid.as<uint8_t>(), cm.ref_valid_rows));
    }
    HIPCHK(hipMemsetAsync(best, 0xFF, un * 8, ctx->stream));  // kCompareNoMatch
    HIPCHK(hipMemsetAsync(sums, 0, kSumWords * 8, ctx->stream));
    const float r2 = max_distance * max_distance;
    if (cm.ref_valid_rows > 0) launch_nearest_across(cm.ref_grid.view(), dc->shared.grid.view(), r2, 0, cm.ref_rows, best, ctx->stream);
    launch_compare_quantise_sum(best, cm.ref_valid.as<uint8_t>(), cm.ref_rows, std::ldexp(1.0f, 18 - dense_radius_exponent(max_distance)), float_bits(r2),
                                cm.dist[1].as<float>(), cm.index[1].as<int32_t>(), sums + dmsa::kAlignPlaneSums, ctx->stream);
    launch_align_plane_sums(best, cm.ref.as<float4>(), cm.ref_valid.as<uint8_t>(), dc->store.g.as<float4>(), dc->normals.normal.as<float4>(), dc->store.n, cm.ref_rows,
                            (float)dmsa_dense_align_scale(dc->cfg.voxel_size), sums, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(al.back.produced(kSlot, ctx->stream));
    HIPCHK(al.back.copy_back(kSlot, kSumWords * 8, ctx->stream2));
    const void* rows = nullptr;
    HIPCHK(al.back.wait_copied(kSlot, &rows));  // the one host read of the sums
    *words = static_cast<const unsigned long long*>(rows);
    return DMSA_OK;
}

// D4's block as read back and D5 of it (the histogram and `within` at tolerance = max_distance)
int fill_direction(dmsa_dense_cloud* dc, const unsigned long long* h, float max_distance, dmsa_dense_compare_direction* d) {
    *d = dmsa_dense_compare_direction{};
    d->queries = dc->compare.ref_valid_rows, d->matched = (int64_t)h[CM_MATCHED], d->unmatched = (int64_t)h[CM_UNMATCHED], d->within = (int64_t)h[CM_WITHIN];
    d->s1 = (int64_t)h[CM_S1], d->s2 = (int64_t)h[CM_S2];
    for (int b = 0; b < DMSA_COMPARE_BINS; ++b) d->histogram[b] = (int64_t)h[CM_BINS + b];
    const double scale = std::ldexp(1.0, 18 - dense_radius_exponent(max_distance));
    if (dmsa_dense_compare_summary(d->matched, d->s1, d->s2, d->within, d->queries, scale, &d->mean_m, &d->rms_m, &d->fraction_within) != DMSA_OK)
        return refuse(dc, "the sums of D4 left their range");  // (never: D1)
    return DMSA_OK;
}

// P1-P7 with the raw rows on the device; T = T_0 on entry and the result on return
int iterate(dmsa_dense_cloud* dc, const float* d_raw, int64_t n, int32_t stride_floats, const dmsa_dense_align_plane_config* cfg, double* T,
            dmsa_dense_align_plane_report* rep) {
    const double scale_c = dmsa_dense_align_scale(dc->cfg.voxel_size);
    rep->scale_c = scale_c, rep->stop = DMSA_ALIGN_STOP_MAX_ITERATIONS;
    bool moved = false;  // T is past the transform the reference stands at
    for (int k = 0; k < cfg->max_iterations; ++k) {
        CHK(dense_reference_from_device_rows(dc, d_raw, n, stride_floats, T));
        moved = false;
        const unsigned long long* h = nullptr;
        CHK(plane_sums(dc, cfg->max_distance, &h));
        for (int w = 0; w < DMSA_ALIGN_PLANE_SUMS; ++w) rep->sums[w] = (int64_t)h[w];
        dmsa_dense_compare_direction d4;
        CHK(fill_direction(dc, h + dmsa::kAlignPlaneSums, cfg->max_distance, &d4));
        dmsa_dense_align_plane_iteration& it = rep->history[k];
        const int64_t used = rep->sums[0], ee_lo = rep->sums[62], ee_hi = rep->sums[63];
        it.matched = d4.matched, it.unmatched = d4.unmatched, it.s2 = d4.s2, it.rms_m = d4.rms_m, it.used = used, it.no_normal = rep->sums[1];
        rep->iterations = k + 1;
        if (used + it.no_normal != d4.matched) return fail(dc->ctx, DMSA_ERR_HIP, "dense align plane: the pairs of P2 and of D4 disagree");  // (never)
        if (used > 0) it.plane_rms_m = std::sqrt((double)((__int128)ee_hi * ((__int128)1 << 32) + (__int128)ee_lo) / (double)used) / (scale_c * 16384.0);
        if (used < cfg->min_pairs) {
            rep->stop = DMSA_ALIGN_STOP_TOO_FEW_PAIRS;
            break;
        }
        double dT[12];
        const int rc = dmsa_dense_align_plane_solve(rep->sums, scale_c, dT, &it.shift_m, &it.rotation_rad, &it.min_pivot);
        if (rc == DMSA_ALIGN_PLANE_DEGENERATE) {
            rep->stop = DMSA_ALIGN_STOP_DEGENERATE;
            break;
        }
        if (rc != DMSA_OK) return refuse(dc, "the sums of P2 left their range");  // (never)
        (void)dmsa_dense_align_compose(dT, T, T);
        moved = true;
        if (it.shift_m <= cfg->stop_translation && it.rotation_rad <= cfg->stop_rotation) {
            rep->stop = DMSA_ALIGN_STOP_CONVERGED;
            break;
        }
    }
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(T[i])) return refuse(dc, "the transform left the finite range");  // (a step is a rotation and a shift; a near-singular system can make that shift huge)
    if (moved) CHK(dense_reference_from_device_rows(dc, d_raw, n, stride_floats, T));  // P8
    return DMSA_OK;
}

}  // namespace

extern "C" {

int dmsa_dense_cloud_align_reference_plane(dmsa_dense_cloud* dc, const float* xyz, int64_t n, int32_t stride_floats, const double* T0,
                                           const dmsa_dense_align_plane_config* cfg, double* T_out, dmsa_dense_align_plane_report* report) {
    if (report) *report = dmsa_dense_align_plane_report{};
    if (!dc || !cfg) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    drop_reference(dc);  // P0: a refused or failed call leaves none
    if (n < 1 || !xyz) return refuse(dc, "a reference of less than one row, or rows without a pointer");
    if (stride_floats < 3) return refuse(dc, "stride_floats must be at least 3");
    if (n > kMaxReference) return refuse(dc, "more than 2^26 reference rows");
    double T[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (T0)
        for (int i = 0; i < 12; ++i) {
            if (!std::isfinite(T0[i])) return refuse(dc, "the transform is not finite");
            T[i] = T0[i];
        }
    CHK(check_store(dc, cfg->max_distance));
    if (const char* why = dense_align_plane_config_refusal(cfg)) return refuse(dc, why);
    CHK(set_device(ctx));
    const size_t bytes = (size_t)n * (size_t)stride_floats * 4;
    DevBuf raw;  // the caller's rows as they came, on the device for the duration of the call
    HIPCHK(raw.ensure(bytes));
    HIPCHK(hipMemcpyAsync(raw.p, xyz, bytes, hipMemcpyHostToDevice, ctx->stream));
    dmsa_dense_align_plane_report rep{};
    const int rc = iterate(dc, raw.as<float>(), n, stride_floats, cfg, T, &rep);
    if (rc != DMSA_OK) {
        (void)hipStreamSynchronize(ctx->stream);  // nothing of a failed call may still read `raw` or the caller's rows
        (void)hipStreamSynchronize(ctx->stream2);
        drop_reference(dc);
        return rc;
    }
    std::memcpy(rep.T, T, sizeof T);
    if (T_out) std::memcpy(T_out, T, sizeof T);
    if (report) *report = rep;
    return DMSA_OK;
}

int dmsa_dense_cloud_align_plane_sums(dmsa_dense_cloud* dc, const dmsa_dense_align_plane_config* cfg, int64_t sums[DMSA_ALIGN_PLANE_SUMS], dmsa_dense_compare_direction* d4) {
    if (d4) *d4 = dmsa_dense_compare_direction{};
    if (!dc || !cfg || !sums) return DMSA_ERR_INVALID;
    CHK(check_store(dc, cfg->max_distance));
    if (dc->compare.ref_rows < 1) return refuse(dc, "no reference cloud (dmsa_dense_cloud_set_reference first)");
    if (dc->compare.ref_valid_rows < 1) return refuse(dc, "the reference cloud has no valid row");
    CHK(set_device(dc->ctx));
    const unsigned long long* h = nullptr;
    CHK(plane_sums(dc, cfg->max_distance, &h));
    for (int w = 0; w < DMSA_ALIGN_PLANE_SUMS; ++w) sums[w] = (int64_t)h[w];
    dmsa_dense_compare_direction d;
    CHK(fill_direction(dc, h + dmsa::kAlignPlaneSums, cfg->max_distance, &d));
    if (d4) *d4 = d;
    return DMSA_OK;
}

}  // extern "C"
