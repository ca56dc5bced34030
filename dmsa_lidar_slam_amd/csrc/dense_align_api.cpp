// dense_align_api.cpp — include/dmsa_dense_align.h (point to point, A0-A8) and include/dmsa_dense_align_plane.h (point to plane, P0-P9) on
// top of dense_align.hip and the pair pass of dense_compare_api.cpp.  Written once over a description of the metric (PointMetric,
// PlaneMetric: the prefix of a refusal, the word count, the floor of min_pairs, what the metric needs of the store, its sums kernel and its
// step from the sums): the checks of A0 / P0, the launch sequence of one iteration's sums (D4's block of the pairs in the completeness
// direction, the metric's sums of the same pairs, one copy back through the stage's CopyBack), and the loop on the context's stream: per
// iteration the reference transformed from the raw rows (dense_compare_api.cpp: D0's own path, which waits for the count of invalid rows
// that the grid's build needs), the sums, then on the host the step (dense_align_solve.cpp, dense_align_plane_solve.cpp), A5's composition
// and the stopping rules of A6 / P7.
#include "dense_cloud_obj.h"

#include "dense_align.h"

#include <cstring>

namespace {

constexpr size_t kMaxSumWords = (size_t)dmsa::kAlignPlaneSums + CM_COUNT;  // the larger block: DenseAlign's one slot holds either
constexpr int kGoOn = -1;                                                   // what a step leaves in *stop beside a DMSA_ALIGN_STOP_*

int refuse(dmsa_dense_cloud* dc, const char* what, const std::string& why) { return fail(dc->ctx, DMSA_ERR_INVALID, std::string(what) + ": " + why); }

// A metric's step(): from an iteration's words and D4's block of its pairs the iteration's own fields and, with *stop = kGoOn, the step dT;
// or *stop = the reason why none is taken; or an error.
struct PointMetric {
    typedef dmsa_dense_align_config Config;
    typedef dmsa_dense_align_iteration Iteration;
    typedef dmsa_dense_align_report Report;
    static constexpr const char* kWhat = "dense align";
    static constexpr int kWords = dmsa::kAlignSums;  // A2's 25 words
    static constexpr int kLeastPairs = 3;
    static int store_ready(dmsa_dense_cloud*) { return DMSA_OK; }
    static void launch_sums(dmsa_dense_cloud* dc, unsigned long long* sums) {
        const DenseCompare& cm = dc->compare;
        launch_align_pair_sums(cm.best[1].as<unsigned long long>(), cm.ref.as<float4>(), cm.ref_valid.as<uint8_t>(), dc->store.g.as<float4>(), dc->store.n, cm.ref_rows,
                               (float)dmsa_dense_align_scale(dc->cfg.voxel_size), sums, dc->ctx->stream);
    }
    static int step(dmsa_dense_cloud* dc, const int64_t* sums, const dmsa_dense_compare_direction& d4, const Config* cfg, double scale_c, Iteration* it, double* dT, int* stop) {
        if (sums[0] != d4.matched) return fail(dc->ctx, DMSA_ERR_HIP, "dense align: the pairs of A2 and of D4 disagree");  // (never)
        if (sums[0] < cfg->min_pairs) return *stop = DMSA_ALIGN_STOP_TOO_FEW_PAIRS, DMSA_OK;
        if (dmsa_dense_align_solve(sums, scale_c, dT, &it->shift_m, &it->rotation_rad) != DMSA_OK) return refuse(dc, kWhat, "the sums of A2 left their range");  // (never)
        return DMSA_OK;
    }
};

struct PlaneMetric {
    typedef dmsa_dense_align_plane_config Config;
    typedef dmsa_dense_align_plane_iteration Iteration;
    typedef dmsa_dense_align_plane_report Report;
    static constexpr const char* kWhat = "dense align plane";
    static constexpr int kWords = dmsa::kAlignPlaneSums;  // P2's 64 words
    static constexpr int kLeastPairs = 6;
    static int store_ready(dmsa_dense_cloud* dc) {  // P0 of the normals
        if (!dc->normals.valid || dc->normals.normal.cap < (size_t)dc->store.n * 16)
            return refuse(dc, kWhat, "no normals of the store as it stands (dmsa_dense_cloud_compute_normals first)");
        return DMSA_OK;
    }
    static void launch_sums(dmsa_dense_cloud* dc, unsigned long long* sums) {
        const DenseCompare& cm = dc->compare;
        launch_align_plane_sums(cm.best[1].as<unsigned long long>(), cm.ref.as<float4>(), cm.ref_valid.as<uint8_t>(), dc->store.g.as<float4>(),
                                dc->normals.normal.as<float4>(), dc->store.n, cm.ref_rows, (float)dmsa_dense_align_scale(dc->cfg.voxel_size), sums, dc->ctx->stream);
    }
    static int step(dmsa_dense_cloud* dc, const int64_t* sums, const dmsa_dense_compare_direction& d4, const Config* cfg, double scale_c, Iteration* it, double* dT, int* stop) {
        const int64_t used = sums[0], ee_lo = sums[62], ee_hi = sums[63];
        it->used = used, it->no_normal = sums[1];
        if (used + it->no_normal != d4.matched) return fail(dc->ctx, DMSA_ERR_HIP, "dense align plane: the pairs of P2 and of D4 disagree");  // (never)
        if (used > 0) it->plane_rms_m = std::sqrt((double)((__int128)ee_hi * ((__int128)1 << 32) + (__int128)ee_lo) / (double)used) / (scale_c * 16384.0);
        if (used < cfg->min_pairs) return *stop = DMSA_ALIGN_STOP_TOO_FEW_PAIRS, DMSA_OK;
        const int rc = dmsa_dense_align_plane_solve(sums, scale_c, dT, &it->shift_m, &it->rotation_rad, &it->min_pivot);
        if (rc == DMSA_ALIGN_PLANE_DEGENERATE) return *stop = DMSA_ALIGN_STOP_DEGENERATE, DMSA_OK;
        return rc != DMSA_OK ? refuse(dc, kWhat, "the sums of P2 left their range") : DMSA_OK;  // (never)
    }
};

// what A0 and P0 ask of the config alone, max_distance apart: the reason of the first breach, or empty
template <class Config>
std::string config_refusal(const Config* cfg, int least_pairs) {
    if (cfg->max_iterations < 1 || cfg->max_iterations > DMSA_ALIGN_MAX_ITERATIONS) return "max_iterations must lie in [1, 64]";
    if (cfg->min_pairs < least_pairs) return "min_pairs must be at least " + std::to_string(least_pairs);
    if (!std::isfinite(cfg->stop_translation) || cfg->stop_translation < 0.0) return "stop_translation must be finite and >= 0";
    if (!std::isfinite(cfg->stop_rotation) || cfg->stop_rotation < 0.0) return "stop_rotation must be finite and >= 0";
    return std::string();
}

// D1 of max_distance and of the store, and what the metric asks of the store
template <class M>
int check_store(dmsa_dense_cloud* dc, float max_distance) {
    CHK(dense_reach_preconditions(dc, max_distance, "max_distance", M::kWhat));
    CHK(dense_row_cap(dc, M::kWhat));
    return M::store_ready(dc);
}

// The metric's sums and D4 of the reference as it stands against the store as it stands, waited for: *words = M::kWords words, then D4's
// block of the same pairs (its `within` at tolerance = max_distance), which the host may read until the next call of this stage
template <class M>
int metric_sums(dmsa_dense_cloud* dc, float max_distance, const unsigned long long** words) {
    constexpr size_t kBytes = ((size_t)M::kWords + CM_COUNT) * 8;
    dmsa_ctx* ctx = dc->ctx;
    DenseAlign& al = dc->align;
    if (!al.created) {
        HIPCHK(al.back.create());
        al.created = true;
    }
    HIPCHK(al.back.reserve(0, kMaxSumWords * 8, kMaxSumWords * 8));
    unsigned long long* sums = al.back.dev[0].as<unsigned long long>();
    HIPCHK(hipMemsetAsync(sums, 0, kBytes, ctx->stream));
    CHK(dense_enqueue_pairs(dc, 1, 0, dc->compare.ref_rows, max_distance, float_bits(max_distance * max_distance), sums + M::kWords));
    M::launch_sums(dc, sums);
    HIPCHK(hipGetLastError());
    HIPCHK(al.back.produced(0, ctx->stream));
    HIPCHK(al.back.copy_back(0, kBytes, ctx->stream2));
    const void* rows = nullptr;
    HIPCHK(al.back.wait_copied(0, &rows));  // the one host read of the sums
    *words = static_cast<const unsigned long long*>(rows);
    return DMSA_OK;
}

// the words as the caller's int64 and D4's block with D5 of it
template <class M>
int read_sums(dmsa_dense_cloud* dc, float max_distance, int64_t* sums, dmsa_dense_compare_direction* d4) {
    const unsigned long long* h = nullptr;
    CHK(metric_sums<M>(dc, max_distance, &h));
    for (int w = 0; w < M::kWords; ++w) sums[w] = (int64_t)h[w];
    return dense_fill_direction(dc, h + M::kWords, dc->compare.ref_valid_rows, std::ldexp(1.0, 18 - dense_radius_exponent(max_distance)), M::kWhat, d4);
}

// A1-A6 / P1-P7 with the raw rows on the device; T = T_0 on entry and the result on return
template <class M>
int iterate(dmsa_dense_cloud* dc, const float* d_raw, int64_t n, int32_t stride_floats, const typename M::Config* cfg, double* T, typename M::Report* rep) {
    const double scale_c = dmsa_dense_align_scale(dc->cfg.voxel_size);
    rep->scale_c = scale_c, rep->stop = DMSA_ALIGN_STOP_MAX_ITERATIONS;
    bool moved = false;  // T is past the transform the reference stands at
    for (int k = 0; k < cfg->max_iterations; ++k) {
        CHK(dense_reference_from_device_rows(dc, d_raw, n, stride_floats, T));
        moved = false;
        dmsa_dense_compare_direction d4;
        CHK(read_sums<M>(dc, cfg->max_distance, rep->sums, &d4));
        typename M::Iteration& it = rep->history[k];
        it.matched = d4.matched, it.unmatched = d4.unmatched, it.s2 = d4.s2, it.rms_m = d4.rms_m;
        rep->iterations = k + 1;
        double dT[12];
        int stop = kGoOn;
        CHK(M::step(dc, rep->sums, d4, cfg, scale_c, &it, dT, &stop));
        if (stop != kGoOn) {
            rep->stop = stop;
            break;
        }
        (void)dmsa_dense_align_compose(dT, T, T);
        moved = true;
        if (it.shift_m <= cfg->stop_translation && it.rotation_rad <= cfg->stop_rotation) {
            rep->stop = DMSA_ALIGN_STOP_CONVERGED;
            break;
        }
    }
    for (int i = 0; i < 12; ++i)  // (a step is a rotation and a shift; P4's near-singular system can make that shift huge)
        if (!std::isfinite(T[i])) return refuse(dc, M::kWhat, "the transform left the finite range");
    if (moved) CHK(dense_reference_from_device_rows(dc, d_raw, n, stride_floats, T));  // A7, P8
    return DMSA_OK;
}

template <class M>
int align_reference(dmsa_dense_cloud* dc, const float* xyz, int64_t n, int32_t stride_floats, const double* T0, const typename M::Config* cfg, double* T_out,
                    typename M::Report* report) {
    if (report) *report = typename M::Report{};
    if (!dc || !cfg) return DMSA_ERR_INVALID;
    dmsa_ctx* ctx = dc->ctx;
    dense_drop_reference(dc);  // A7, P0: a refused or failed call leaves none
    CHK(dense_reference_rows_accepted(dc, xyz, n, stride_floats, 1, "a reference of less than one row, or rows without a pointer", M::kWhat));
    double T[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (T0)
        for (int i = 0; i < 12; ++i) {
            if (!std::isfinite(T0[i])) return refuse(dc, M::kWhat, "the transform is not finite");
            T[i] = T0[i];
        }
    CHK(check_store<M>(dc, cfg->max_distance));
    if (const std::string why = config_refusal(cfg, M::kLeastPairs); !why.empty()) return refuse(dc, M::kWhat, why);
    CHK(set_device(ctx));
    DevBuf raw;  // the caller's rows as they came, on the device for the duration of the call
    CHK(dense_upload_reference_rows(dc, xyz, n, stride_floats, &raw));
    typename M::Report rep{};
    const int rc = iterate<M>(dc, raw.as<float>(), n, stride_floats, cfg, T, &rep);
    if (rc != DMSA_OK) {
        (void)hipStreamSynchronize(ctx->stream);  // nothing of a failed call may still read `raw` or the caller's rows
        (void)hipStreamSynchronize(ctx->stream2);
        dense_drop_reference(dc);
        return rc;
    }
    std::memcpy(rep.T, T, sizeof T);
    if (T_out) std::memcpy(T_out, T, sizeof T);
    if (report) *report = rep;
    return DMSA_OK;
}

// the stage call: of cfg only max_distance is read
template <class M>
int align_sums(dmsa_dense_cloud* dc, const typename M::Config* cfg, int64_t* sums, dmsa_dense_compare_direction* d4) {
    if (d4) *d4 = dmsa_dense_compare_direction{};
    if (!dc || !cfg || !sums) return DMSA_ERR_INVALID;
    CHK(check_store<M>(dc, cfg->max_distance));
    if (dc->compare.ref_rows < 1) return refuse(dc, M::kWhat, "no reference cloud (dmsa_dense_cloud_set_reference first)");
    if (dc->compare.ref_valid_rows < 1) return refuse(dc, M::kWhat, "the reference cloud has no valid row");
    CHK(set_device(dc->ctx));
    dmsa_dense_compare_direction d;
    CHK(read_sums<M>(dc, cfg->max_distance, sums, &d));
    if (d4) *d4 = d;
    return DMSA_OK;
}

}  // namespace

extern "C" {

int dmsa_dense_cloud_align_reference(dmsa_dense_cloud* dc, const float* xyz, int64_t n, int32_t stride_floats, const double* T0, const dmsa_dense_align_config* cfg,
                                     double* T_out, dmsa_dense_align_report* report) {
    return align_reference<PointMetric>(dc, xyz, n, stride_floats, T0, cfg, T_out, report);
}
int dmsa_dense_cloud_align_sums(dmsa_dense_cloud* dc, const dmsa_dense_align_config* cfg, int64_t sums[DMSA_ALIGN_SUMS], dmsa_dense_compare_direction* d4) {
    return align_sums<PointMetric>(dc, cfg, sums, d4);
}

int dmsa_dense_cloud_align_reference_plane(dmsa_dense_cloud* dc, const float* xyz, int64_t n, int32_t stride_floats, const double* T0,
                                           const dmsa_dense_align_plane_config* cfg, double* T_out, dmsa_dense_align_plane_report* report) {
    return align_reference<PlaneMetric>(dc, xyz, n, stride_floats, T0, cfg, T_out, report);
}
int dmsa_dense_cloud_align_plane_sums(dmsa_dense_cloud* dc, const dmsa_dense_align_plane_config* cfg, int64_t sums[DMSA_ALIGN_PLANE_SUMS], dmsa_dense_compare_direction* d4) {
    return align_sums<PlaneMetric>(dc, cfg, sums, d4);
}

}  // extern "C"
