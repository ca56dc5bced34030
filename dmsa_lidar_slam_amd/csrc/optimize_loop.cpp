// optimize_loop.cpp — DmsaOptimizer::optimizeSet (DmsaOptimizer.h:54-150): pose tables, residual batches, the analytic Jacobian, what the two
// loops share, the host-driven loop (host-built pose tables, debug switch device_loop = 0, sets too large for the chain kernels' LDS), the
// device-resident loop (default) as a plan (LoopPlan: every mode of a call, decided once), its buffers and named phases, and optimize().
#include "dmsa_ctx.h"

// ---- pose tables ------------------------------------------------------------------------------------------
// `globs`: B x (C or F) x 6 doubles (axis-angle | translation) of the GLOBAL poses of every evaluation in the batch.
int build_tables(dmsa_ctx* ctx, int B, const std::vector<double>& globs, hipStream_t stream) {
    if (stream == nullptr) stream = ctx->stream;
    if (stream == ctx->stream) CHK(ctx->tables.wait_owed(ctx->stream));  // an earlier batch's tables may still be in flight on the side stream
    ScopedTimer tm(ctx, T_TABLE);
    const int rows = ctx->rows;
    HIPCHK(ctx->d_tables.ensure((size_t)B * rows * 48));
    const int np = ctx->model == MODEL_WINDOW ? ctx->win.ctrl.n : ctx->key.frames.n;
    if (ctx->flags & DMSA_FLAG_POSE_TABLE_HOST) {
        ctx->h_tables.resize((size_t)B * rows * 12);
        auto build_range = [&](int b0, int b1) {
            PoseChain tmp;
            tmp.resize(np);
            for (int b = b0; b < b1; ++b) {
                for (int k = 0; k < np; ++k)
                    for (int c = 0; c < 3; ++c) {
                        tmp.glob_o[3 * k + c] = globs[((size_t)b * np + k) * 6 + c];
                        tmp.glob_t[3 * k + c] = globs[((size_t)b * np + k) * 6 + 3 + c];
                    }
                float* T = &ctx->h_tables[(size_t)b * rows * 12];
                if (ctx->model == MODEL_WINDOW)
                    window_dense_table(tmp, ctx->win.stamps, ctx->win.fh, ctx->win.traj_time, T);
                else
                    keyframe_table(tmp, T);
                float* id = T + (size_t)(rows - 1) * 12;  // identity row used by static points
                const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
                std::memcpy(id, I, sizeof(I));
            }
        };
        // every table is a pure function of its control poses: build the tables of a batch on several host threads
        if ((size_t)B * rows < 4096) {
            build_range(0, B);
        } else {
            workers(ctx).run_all([&](int t, int nt) { build_range((int)((int64_t)B * t / nt), (int)((int64_t)B * (t + 1) / nt)); });
        }
        HIPCHK(hipMemcpyAsync(ctx->d_tables.p, ctx->h_tables.data(), ctx->h_tables.size() * 4, hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));  // h_tables is reused by the next batch
    } else {
        HIPCHK(ctx->d_ctrl.ensure(globs.size() * 8));
        double* slot = nullptr;
        HIPCHK(ctx->h_pin.next(globs.size(), ctx->stream, &slot));
        std::memcpy(slot, globs.data(), globs.size() * 8);
        HIPCHK(hipMemcpyAsync(ctx->d_ctrl.p, slot, globs.size() * 8, hipMemcpyHostToDevice, stream));
        // default path: the correspondence kernels read the tables transposed ([row][evaluation][12]); batches are written both ways at once
        float* tT = nullptr;
        if (B > 1) {
            HIPCHK(ctx->d_tablesT.ensure((size_t)B * rows * 48));
            tT = ctx->d_tablesT.as<float>();
        }
        if (ctx->model == MODEL_WINDOW)
            launch_window_pose_tables(ctx->d_ctrl.as<double>(), ctx->d_stamps.as<double>(), ctx->d_fhw.as<double>(), ctx->d_trajtime.as<double>(), B,
                                      np, rows - 1, ctx->d_tables.as<float>(), tT, stream);
        else
            launch_keyframe_pose_tables(ctx->d_ctrl.as<double>(), B, np, ctx->d_tables.as<float>(), tT, stream);
        ctx->batch = B;
        ctx->tablesT_batch = tT ? B : 0;
        return DMSA_OK;
    }
    ctx->batch = B;
    ctx->tablesT_batch = 0;  // the transposed copy (default path) no longer matches
    return DMSA_OK;
}
// pose tables of B control-pose sets that are on the device already (device loop)
static int device_tables(dmsa_ctx* ctx, int B, const double* d_ctrl, float* tables, float* tablesT, hipStream_t stream, uint32_t* rot_same = nullptr) {
    const int np = ctx->loop_model.n;
    if (ctx->model == MODEL_WINDOW)
        launch_window_pose_tables(d_ctrl, ctx->d_stamps.as<double>(), ctx->d_fhw.as<double>(), ctx->d_trajtime.as<double>(), B, np, ctx->rows - 1, tables, tablesT,
                                  stream, rot_same);
    else
        launch_keyframe_pose_tables(d_ctrl, B, np, tables, tablesT, stream, rot_same);
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}
// a slot of the pinned ring the control poses go through
static int pinned_doubles(dmsa_ctx* ctx, size_t count, double** out) {
    HIPCHK(ctx->h_pin.next(count, ctx->stream, out));
    return DMSA_OK;
}

void append_glob(const PoseChain& c, std::vector<double>& out) {
    for (int k = 0; k < c.n; ++k) {
        for (int a = 0; a < 3; ++a) out.push_back(c.glob_o[3 * k + a]);
        for (int a = 0; a < 3; ++a) out.push_back(c.glob_t[3 * k + a]);
    }
}

// one forward evaluation's host part for the CURRENT chain state: record global poses, compute additional rows
static void host_eval(dmsa_ctx* ctx, std::vector<double>& globs, std::vector<double>& extra) {
    append_glob(chain(ctx), globs);
    const int a = num_extra_rows(ctx);
    if (a > 0) {
        const size_t at = extra.size();
        extra.resize(at + a);
        if (ctx->model == MODEL_WINDOW)
            ctx->win.imu_rows(&extra[at]);  // runs global_to_relative like updateImuError
        else
            ctx->key.additional_rows(&extra[at]);
    }
    ctx->evaluations += 1;
}
// setPoseParameters + the chain update of updateGlobalPoints for both models
void host_set_params(dmsa_ctx* ctx, const double* p) {
    chain(ctx).set_params(p);
    chain(ctx).relative_to_global();
}

int transform_points(dmsa_ctx* ctx, int b) {
    const float4* table = ctx->d_tables.as<float4>() + (size_t)b * ctx->rows * 3;
    ctx->base_table = reinterpret_cast<const float*>(table);  // the fit re-derives the global coordinates of the members from this table
    if (ctx->model == MODEL_KEYFRAMES)
        launch_transform_normals(ctx->d_local.as<float4>(), ctx->d_nlocal.as<float4>(), table, ctx->d_global.as<float4>(), ctx->d_nglobal.as<float4>(),
                                 ctx->n, ctx->stream);
    else
        launch_transform(ctx->d_local.as<float4>(), table, ctx->d_global.as<float4>(), ctx->n, ctx->stream);
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}


// ---- residual batches ----------------------------------------------------------------------------------------
int ensure_E(dmsa_ctx* ctx, int B) {
    const int a = num_extra_rows(ctx);
    ctx->extra_rows = a;
    const int64_t ld = (((int64_t)ctx->M + a) + 31) / 32 * 32;
    ctx->ldE = ld;
    HIPCHK(ctx->d_E.ensure((size_t)B * ld * 8));
    return DMSA_OK;
}
int upload_extra(dmsa_ctx* ctx, const std::vector<double>& extra, int B) {
    // additional rows (IMU / gravity / odometry) go below the Gaussian rows of every evaluation, through a pinned ring like the
    // control poses: no host synchronisation, and the copy runs ahead of the correspondence kernels
    const int a = ctx->extra_rows;
    const size_t need = (size_t)a * B;
    double* slot = nullptr;
    HIPCHK(ctx->h_xpin.next(need, ctx->stream, &slot));
    std::memcpy(slot, extra.data(), need * sizeof(double));
    HIPCHK(hipMemcpy2DAsync(ctx->d_E.as<double>() + ctx->M, (size_t)ctx->ldE * 8, slot, (size_t)a * 8, (size_t)a * 8, (size_t)B, hipMemcpyHostToDevice,
                            ctx->stream));
    return DMSA_OK;
}

// Where the three tiers of a batch run, and how the batch is timed.
struct TierPlan {
    bool two, three;  // the throughput tier on stream2; the short tier on stream3 as well
    hipStream_t s_long, s_mid, s_small;
    BatchStamp stamp;  // ticks != null: the batch is timed by the device's wall clock inside its own kernels
    int serial_tree;
};
static TierPlan plan_tiers(dmsa_ctx* ctx) {
    TierPlan t{};
    t.two = ctx->dbg.serial_streams >= 2 && ctx->serial_counts.n_long > 0;
    t.three = t.two && ctx->dbg.serial_streams >= 3;
    // The latency tier keeps `stream` and is launched first: its workgroups must get their CUs before the thousands of workgroups of
    // the other tiers fill the chip.  (Giving `stream` to the throughput tier in the Jacobian batch, which that tier bounds, so that it
    // starts without the ~12 us fork delay: 1050 -> 990 it/s -- the latency tier then queues behind everybody else.)
    t.s_long = ctx->stream;
    t.s_mid = t.two ? ctx->stream2 : ctx->stream;
    t.s_small = t.three ? ctx->stream3 : t.s_mid;
    // The batch's time (dmsa_timing::residual_kernel_ms).  A batch with a join wait -- tiers on more than one stream, dependencies by counter --
    // takes it from the device's wall clock inside kernels it has anyway (dev_sync.h: BatchStamp): its latency tier, given the fork counter,
    // stamps the begin beside it; the join's wait kernel adds the difference to d_batch_clock.  Every other batch keeps the HIP-event pair
    // around it, whose two barrier packets idle the main stream for 6-7 us each (profiles/r15_iteration_timeline.txt); debug switch
    // batch_stamps = 0: every batch does.
    if (ctx->dbg.batch_stamps != 0 && t.two && ctx->tier_join.by_counter() && ctx->d_batch_clock.p != nullptr)
        t.stamp.begin = reinterpret_cast<const long long*>(ctx->d_sync.as<uint32_t>() + SYNC_BATCH_BEGIN), t.stamp.ticks = ctx->d_batch_clock.as<unsigned long long>();
    t.serial_tree = ctx->dbg.serial_tree;
    return t;
}

// The second pass of the longest Gaussians shared out to helper workgroups (serial_kernels.hip: k_residuals_chain, LongHelp): *split = `store`
// filled in, or null where the rule says no.  A scratch that has to grow is zeroed on the main stream.
static int long_split_for(dmsa_ctx* ctx, int B, LongSplit* store, const LongSplit** split) {
    *split = nullptr;
    // Measured (round 6): where a FEW long Gaussians end a batch (the rosette window: 2 - 3 of them) the helpers take 10 % off the iteration; the
    // bench window's 110 long Gaussians keep ~220 compute units busy side by side and the helpers of the longest ones gain nothing there
    // (1235 -> 1200-1218 it/s), nor for the keyframe sets (4 long Gaussians, B = 187 and 9: 985 -> 953).  Rule: window model, at most 16 long Gaussians (= the Gaussians that get helper blocks), B <= 32;
    // long_split >= 2 = that many members as the threshold, everywhere (experiments).
    const bool split_auto = ctx->dbg.long_split == 1 && ctx->serial_counts.n_long <= 16 && B <= 32 && ctx->model == MODEL_WINDOW;
    if (!((split_auto || ctx->dbg.long_split >= 2) && ctx->serial_counts.n_long > 0 && ctx->dbg.serial_tree != 0)) return DMSA_OK;
    const SerialShape shp = serial_shape(B);
    const size_t items = (size_t)ctx->serial_counts.n_long * shp.nsub_long;
    store->helpers = 8;
    store->lead_gaussians = 16;
    // few long Gaussians (rosette window, keyframe sets): every one of them may hand over; many (the bench window has 110): the longest
    store->min_members = ctx->dbg.long_split >= 2 ? ctx->dbg.long_split : 0;  // (auto: every Gaussian of the latency tier)
    const size_t H = (size_t)store->helpers;
    if (items > ctx->long_split_items) {  // layout by CAPACITY: the tickets keep their place (and their zeros) when the item count changes between batches
        const size_t cap = items + items / 2 + 16;
        HIPCHK(ctx->d_long_split.ensure(cap * (8 + 48 * 4 + H * 16 * 12) + 64));
        HIPCHK(hipMemsetAsync(ctx->d_long_split.p, 0, ctx->d_long_split.cap, ctx->stream));  // tickets at zero, flags below every epoch
        ctx->long_split_items = cap;
    }
    const size_t cap = ctx->long_split_items;
    char* w = ctx->d_long_split.as<char>();
    store->partial = reinterpret_cast<double*>(w), w += cap * H * 16 * 8;
    store->means = reinterpret_cast<float*>(w), w += cap * 48 * 4;
    store->partial_key = reinterpret_cast<int*>(w), w += cap * H * 16 * 4;
    store->done = reinterpret_cast<uint32_t*>(w), w += cap * 4;
    store->ready = reinterpret_cast<uint32_t*>(w);
    store->timed_out = StreamDep::timed_out(ctx);
    store->epoch = next_epoch(ctx->long_split_epoch);
    *split = store;
    return DMSA_OK;
}

// The correspondence kernels of one batch (reference-order sums: lane = evaluation on transposed pose tables): what every launch of the
// batch shares, stated once.  Launches differ in the fork signal the latency tier carries, in the tiers they hold (bit 0: latency, bit 1:
// throughput, bit 2: short) and in whether the latency tier's second pass is split.
struct SerialBatch {
    dmsa_ctx* ctx;
    int B;
    const TierPlan& t;
    const uint32_t* rot_same;
    const int2* row_range;
    const int2* gauss_rows;
    void launch(uint32_t* fork_signal, int tiers, const LongSplit* split) const {
        launch_residuals_serial(ctx->d_memb_local.as<float4>(), ctx->d_seg_off.as<int32_t>(), ctx->d_info12.as<float>(), ctx->d_tablesT.as<float>(), B,
                                ctx->d_order.as<uint32_t>(), ctx->serial_counts, ctx->d_E.as<double>(), ctx->ldE, t.s_long, t.s_mid, t.s_small, t.serial_tree,
                                fork_signal, tiers, rot_same, row_range, gauss_rows, split);
    }
};
// Fork and join of the tier streams: counters in device memory (loop_kernels.h) instead of events, whose barrier packets cost 8-10 us per
// record / wait on `stream`; debug switch device_sync = 0 keeps the events.
// The fork.  Counters (`counter_signal`: the latency tier, already launched, gives the signal itself once all its workgroups are placed,
// serial_kernels.hip -- its launch is enqueued before these waits, the order that rules out a deadlock on shared hardware queues, dev_sync.h
// rule (1)): the waits in front of the other tiers.  Events: the fork is recorded here, in front of all three tiers.
static int fork_tiers(dmsa_ctx* ctx, const TierPlan& t, bool counter_signal) {
    if (!counter_signal) CHK(ctx->tier_fork.signal(ctx->stream, t.s_mid));
    CHK(ctx->tier_fork.wait(t.s_mid, ctx->stream));
    if (t.three) CHK(ctx->tier_fork.wait(t.s_small, ctx->stream));
    return DMSA_OK;
}
static int join_tiers(dmsa_ctx* ctx, const TierPlan& t) {
    if (ctx->tier_join.by_counter()) {  // one counter collects both tier streams
        CHK(ctx->tier_join.signal(t.s_mid, ctx->stream));
        if (t.three) CHK(ctx->tier_join.signal(t.s_small, ctx->stream));
        WaitCarry end;
        end.stamp = t.stamp;
        return ctx->tier_join.wait(ctx->stream, t.s_mid, 0, &end);
    }
    // events: the stream that finishes first is waited for first (its wait is through while `stream` still works)
    if (t.three) {
        CHK(ctx->tier_join.signal(t.s_small, ctx->stream, 1));
        CHK(ctx->tier_join.wait(ctx->stream, t.s_small, 1));
    }
    CHK(ctx->tier_join.signal(t.s_mid, ctx->stream));
    return ctx->tier_join.wait(ctx->stream, t.s_mid);
}
int run_residuals(dmsa_ctx* ctx, int B, const std::vector<double>* extra, const double* d_extra, const uint32_t* rot_same, const int2* row_range) {
    CHK(ensure_E(ctx, B));
    CHK(ctx->tables.wait_owed(ctx->stream));  // the pose tables of this batch were built on another stream (and k_size_classes did not wait for them)
    const int a = ctx->extra_rows;
    if (a > 0 && d_extra != nullptr)  // device loop: the chain kernels left the additional rows of the batch in device memory
        launch_loop_scatter_extra(d_extra, B, a, ctx->d_E.as<double>(), ctx->ldE, ctx->M, ctx->stream);
    if (a > 0 && extra != nullptr) CHK(upload_extra(ctx, *extra, B));
    if (!ctx->order_valid) {
        ctx->err = "residuals: no size-class order (build the Gaussians first)";
        return DMSA_ERR_INVALID;
    }
    {
        HIPCHK(ctx->d_tablesT.ensure((size_t)B * ctx->rows * 48));
        const TierPlan t = plan_tiers(ctx);
        if (t.stamp.ticks != nullptr) ctx->batch_ticks_dirty = true;
        ScopedTimer tm(ctx, T_RESIDUAL, t.stamp.ticks != nullptr);
        if (ctx->tablesT_batch != B) launch_transpose_tables(ctx->d_tables.as<float>(), ctx->rows, B, ctx->d_tablesT.as<float>(), ctx->stream);
        const SerialBatch batch{ctx, B, t, rot_same, row_range, row_range ? ctx->d_gauss_rows.as<int2>() : nullptr};
        uint32_t* fork_signal = ctx->tier_fork.kernel_signal(ctx->stream, t.s_mid);  // (null: events, or one stream)
        if (fork_signal == nullptr) CHK(fork_tiers(ctx, t, false));
        LongSplit split_store;
        const LongSplit* split = nullptr;
        CHK(long_split_for(ctx, B, &split_store, &split));
        if (fork_signal != nullptr) {  // latency tier first (with the signal), then the waits in front of the other tiers
            batch.launch(fork_signal, 1, split);
            CHK(fork_tiers(ctx, t, true));
            batch.launch(nullptr, 6, nullptr);
        } else {
            batch.launch(nullptr, 7, split);
        }
        CHK(join_tiers(ctx, t));
    }
    ctx->E_is_jacobian = false;
    ctx->residual_launches += 1;
    ctx->residual_evals += B;
    ctx->residual_bytes += 16.0 * (double)ctx->Mm + 48.0 * ctx->M + (double)B * (48.0 * ctx->rows + 8.0 * ctx->M);
    ctx->residual_unit_bytes += (double)B * (16.0 * (double)ctx->Mm + 56.0 * ctx->M + 48.0 * ctx->rows);
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}


// ---- analytic Jacobian (settings.use_analytic_jacobi) ------------------------------------------------------------------------------------
// Per iteration: evaluation 0, the additional rows of the 1 + P parameter sets (forward differences as before), the pose-table derivatives
// by central differences in fp64 (2P chains, then one kernel) and the Gaussian rows of J from them (analytic_jacobian.h).
int check_analytic_jacobian(dmsa_ctx* ctx, int P) {
    if (P > kAnalyticJacobianMaxP) {
        ctx->err = "use_analytic_jacobi: " + std::to_string(P) + " parameters, the analytic Jacobian takes at most " + std::to_string(kAnalyticJacobianMaxP);
        return DMSA_ERR_INVALID;
    }
    return DMSA_OK;
}
// d_dT from the 2P control-pose sets at d_ctrl_pm
static int table_derivatives(dmsa_ctx* ctx, const double* d_ctrl_pm, hipStream_t stream) {
    const int P = num_params(ctx), np = chain(ctx).n;
    HIPCHK(ctx->d_dT.ensure((size_t)ctx->rows * 12 * P * 8));
    if (ctx->model == MODEL_WINDOW)
        launch_window_pose_table_deriv(d_ctrl_pm, ctx->d_stamps.as<double>(), ctx->d_fhw.as<double>(), ctx->d_trajtime.as<double>(), P, np, ctx->rows - 1,
                                       kTableDerivStep, ctx->d_dT.as<double>(), stream);
    else
        launch_keyframe_pose_table_deriv(d_ctrl_pm, P, np, kTableDerivStep, ctx->d_dT.as<double>(), stream);
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}
// (Not one of keyframe_chains_aside's callers, the builder of perturbed host chains below: this one perturbs a PoseChain of either model, not a
// KeyframeHost, has no additional rows, writes into pinned memory, counts no evaluation, leaves the host chain alone and stays on the calling
// thread for small sets -- sharing the function would take a mode flag for each of these.)
int host_table_derivatives(dmsa_ctx* ctx, hipStream_t stream) {
    const int P = num_params(ctx);
    const PoseChain base = chain(ctx);
    const size_t gsz = (size_t)base.n * 6;
    std::vector<double> p0((size_t)P);
    base.get_params(p0.data());
    double* pin = nullptr;
    CHK(pinned_doubles(ctx, 2 * (size_t)P * gsz, &pin));
    // the chains of k_loop_chain_central, on the host: every set is an independent chain from the same start
    auto build_range = [&](int t, int nt) {
        PoseChain c = base;
        std::vector<double> lp, g;
        for (int b = t; b < 2 * P; b += nt) {
            lp = p0;
            lp[(size_t)(b >> 1)] += (b & 1) ? -kTableDerivStep : kTableDerivStep;
            c.set_params(lp.data());
            c.relative_to_global_smooth();  // no identity cut on the derivative side (pose_math.h: so3_exp<false>)
            g.clear();
            append_glob(c, g);
            std::copy(g.begin(), g.end(), pin + (size_t)b * gsz);
        }
    };
    if ((size_t)P * base.n < 4096)
        build_range(0, 1);
    else
        workers(ctx).run_all(build_range);
    HIPCHK(ctx->d_ctrl_pm.ensure(2 * (size_t)P * gsz * 8));
    HIPCHK(hipMemcpyAsync(ctx->d_ctrl_pm.p, pin, 2 * (size_t)P * gsz * 8, hipMemcpyHostToDevice, stream));
    return table_derivatives(ctx, ctx->d_ctrl_pm.as<double>(), stream);
}
int analytic_columns(dmsa_ctx* ctx, int P, double inv_h, const float* table0) {
    CHK(check_analytic_jacobian(ctx, P));
    double* E = ctx->d_E.as<double>();
    // the additional rows keep the reference's forward differences, bit for bit the numeric path's columns
    if (ctx->extra_rows > 0) launch_jacobian_columns(E + ctx->M, ctx->ldE, ctx->extra_rows, P, inv_h, ctx->stream);
    launch_analytic_jacobian(ctx->d_memb_local.as<float4>(), ctx->d_seg_off.as<int32_t>(), ctx->d_info12.as<float>(), table0, ctx->d_dT.as<double>(), ctx->M, P,
                             ctx->rows - 1, E, ctx->ldE, ctx->stream);
    HIPCHK(hipGetLastError());
    ctx->E_is_jacobian = true;
    return DMSA_OK;
}


// ---- what the two loops share ----------------------------------------------------------------------------------------
// Perturbed parameter sets -> chains on the worker pool -> `globs` (+ additional rows in `extra`) at the evaluation slots slot0 .. slot0 +
// count - 1 of a batch.  The keyframe model carries no state from one evaluation to the next (setPoseParameters rewrites every relative pose
// and re-chains, MapManagement.h:197-202), so the chains (O(F) exp/log each) are built side by side by a few host threads; results are
// identical to the serial order.  params_of(j, p) writes the P parameters of set j.  The host chain is left where the serial loop leaves it:
// at the last set (`last` is the caller's scratch for it), all `count` evaluations counted.
template <class ParamsOf>
static void keyframe_chains_aside(dmsa_ctx* ctx, int P, int count, int slot0, const ParamsOf& params_of, std::vector<double>& globs, std::vector<double>& extra,
                                  std::vector<double>& last) {
    const int a = num_extra_rows(ctx);
    const size_t gsz = (size_t)chain(ctx).n * 6;
    globs.resize((size_t)(slot0 + count) * gsz);
    extra.resize((size_t)(slot0 + count) * a);
    const KeyframeHost base = ctx->key;
    workers(ctx).run_all([&](int t, int nthr) {
        KeyframeHost kh = base;
        std::vector<double> p((size_t)P), g;
        for (int j = t; j < count; j += nthr) {
            params_of(j, p.data());
            kh.frames.set_params(p.data());
            kh.frames.relative_to_global();
            g.clear();
            append_glob(kh.frames, g);
            std::copy(g.begin(), g.end(), globs.begin() + (size_t)(slot0 + j) * gsz);
            if (a > 0) kh.additional_rows(&extra[(size_t)(slot0 + j) * a]);
        }
    });
    ctx->evaluations += count;
    params_of(count - 1, last.data());
    host_set_params(ctx, last.data());
}

// adaptiveStepSize (DmsaOptimizer.h:152-182) on the resident problem and its current Gaussians, host-driven: nine trial evaluations at
// raw + 0.1 k step in one batch; `paramVec` (in: raw) becomes the arg-min if it beats error0 (strict '<'), *bestK its k (0: none -- the set is
// then left at the LAST trial, raw + 0.9 step, like the reference's object, :160-165).  Used by the host-driven loop and by the C ABI's
// dmsa_adaptive_step_size (the reference's method is public, DmsaOptimizer.h:152).
static int host_adaptive_step_size(dmsa_ctx* ctx, int P, std::vector<double>& paramVec, const std::vector<double>& step, double error0, int* bestK_out) {
    std::vector<double> globs, extra, test((size_t)P);
    auto trial = [&](int k, double* out) {
        for (int i = 0; i < P; ++i) out[i] = paramVec[(size_t)i] + 0.1 * (double)k * step[(size_t)i];
    };
    if (ctx->model == MODEL_KEYFRAMES && P >= 48) {
        // like the Jacobian batch: the nine trial chains are built side by side; the chain is left at the last trial evaluated
        keyframe_chains_aside(ctx, P, 9, 0, [&](int j, double* out) { trial(j + 1, out); }, globs, extra, test);
    } else {
        for (int k = 1; k < 10; ++k) {
            trial(k, test.data());
            host_set_params(ctx, test.data());
            host_eval(ctx, globs, extra);
        }
    }
    ctx->tl.mark("trial chains");
    CHK(build_tables(ctx, 9, globs));
    CHK(run_residuals(ctx, 9, &extra));
    // the rows of e^T e: read after run_residuals (ensure_E sets extra_rows for the problem resident NOW -- a value taken before
    // would miss the additional rows after an upload, or count stale ones after a re-upload with another number of them)
    const int rowsE = ctx->M + ctx->extra_rows;
    double* errs = ctx->rb()->errs;  // pinned
    {
        ScopedTimer tm(ctx, T_NORMAL);
        HIPCHK(ctx->d_sq_partial.ensure((size_t)squared_sums_blocked_partial_doubles(rowsE, P, 9) * 8));
        HIPCHK(ctx->d_sq_out.ensure(16 * 8));
        launch_squared_sums_blocked(ctx->d_E.as<double>(), ctx->ldE, rowsE, P, 9, ctx->d_sq_partial.as<double>(), ctx->d_sq_out.as<double>(), ctx->stream);
    }
    HIPCHK(hipMemcpyAsync(errs, ctx->d_sq_out.p, 9 * 8, hipMemcpyDeviceToHost, ctx->stream));
    ctx->tl.mark("line search enq");
    HIPCHK(sync_spin(ctx->stream));  // sync #4
    ctx->tl.mark("sync#4 wait");
    drain_timers(ctx);
    double minError = error0;
    int bestK = 0;
    const std::vector<double> raw = paramVec;
    for (int k = 1; k < 10; ++k)
        if (errs[k - 1] < minError) {
            for (int i = 0; i < P; ++i) paramVec[(size_t)i] = raw[(size_t)i] + 0.1 * (double)k * step[(size_t)i];
            minError = errs[k - 1], bestK = k;
        }
    *bestK_out = bestK;
    return DMSA_OK;
}

// C ABI seam of adaptiveStepSize (include/dmsa_hip.h: dmsa_adaptive_step_size)
int adaptive_step_size(dmsa_ctx* ctx, double* params, const double* step, double error0, int32_t* best_k) {
    if (ctx->model == MODEL_NONE || !ctx->gaussians_valid || !ctx->order_valid) {
        ctx->err = "adaptive_step_size: no Gaussians (dmsa_build_gaussians or an optimize call first)";
        return DMSA_ERR_INVALID;
    }
    const int P = num_params(ctx);
    std::vector<double> pv(params, params + P), st(step, step + P);
    int k = 0;
    CHK(host_adaptive_step_size(ctx, P, pv, st, error0, &k));
    std::copy(pv.begin(), pv.end(), params);
    *best_k = k;
    return DMSA_OK;
}

// :101-113 on the host: the normal equations come back through pinned memory, are split into H and g and damped, and lm_solve takes the
// explicit inverse like the reference (on the worker pool from P = 64 on).  *error0 receives e0^T e0, element (P, P) of Hp; the step is in `step`.
struct HostLmSolve {
    std::vector<double> Hp, H, g, step;
    int run(dmsa_ctx* ctx, const dmsa_settings& s, int P, int solve_threads, const char* wait_mark, double* error0) {
        const int n1 = P + 1;
        Hp.resize((size_t)n1 * n1), H.resize((size_t)P * P), g.resize((size_t)P), step.resize((size_t)P);
        HIPCHK(ctx->h_Hp.ensure(Hp.size() * 8, nullptr));  // (the previous read-back was waited for)
        HIPCHK(hipMemcpyAsync(ctx->h_Hp.p, ctx->d_Hp.p, Hp.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        ctx->tl.mark("residuals+NE enq");
        HIPCHK(sync_spin(ctx->stream));  // sync #3 of the host-driven loop, sync B of the device loop (P > 1024 only)
        ctx->tl.mark(wait_mark);
        std::memcpy(Hp.data(), ctx->h_Hp.p, Hp.size() * 8);
        for (int j = 0; j < P; ++j)
            for (int i = 0; i < P; ++i) H[(size_t)j * P + i] = Hp[(size_t)j * n1 + i];
        for (int i = 0; i < P; ++i) g[(size_t)i] = Hp[(size_t)P * n1 + i];
        *error0 = Hp[(size_t)P * n1 + P];  // :101
        for (int i = 0; i < P; ++i) H[(size_t)i * P + i] += (double)s.lambda_diag;  // :110
        const ParallelRun par = [&](const std::function<void(int, int)>& fn) { workers(ctx).run_all(fn); };
        lm_solve(H.data(), g.data(), P, s.step_length_optim, step.data(), P >= 64 ? &par : nullptr, solve_threads);  // :113
        return DMSA_OK;
    }
};
// the end of a call: back from the centred frame, :149 final updateGlobalPoints, the report
static int finish_call(dmsa_ctx* ctx, const dmsa_settings& s, dmsa_report* rep, int iters, int stop, double error0, double stepNorm, int bestK) {
    if (s.use_centralization) CHK(dmsa_decentralize(ctx));
    // :149 final updateGlobalPoints
    if (ctx->model == MODEL_WINDOW) chain(ctx).relative_to_global();
    std::vector<double> globs;
    append_glob(chain(ctx), globs);
    CHK(build_tables(ctx, 1, globs));
    CHK(transform_points(ctx, 0));
    HIPCHK(enqueue_batch_ticks(ctx));  // (host-driven loop; the device loop's rode on its own last copies)
    HIPCHK(hipStreamSynchronize(ctx->stream));
    // A NaN e0^T e0 (a NaN measurement in an additional row) is reported as THE quiet NaN.  Which NaN arithmetic hands on is the processor's
    // choice: pose_math.h's `dp - preint_pos` is an add with a negated operand on gfx950, which flips the sign of a NaN preint_pos, and a subsd on
    // x86, which keeps it -- the device loop and the host-driven loop returned different bits for the same call, and only the latter the reference's.
    if (std::isnan(error0)) error0 = std::numeric_limits<double>::quiet_NaN();
    if (rep) {
        rep->iterations = iters, rep->stop_reason = stop;
        rep->num_gaussians = ctx->M, rep->num_gaussians_l1 = ctx->M1, rep->num_memberships = ctx->Mm;
        rep->error0 = error0, rep->last_step_norm = stepNorm, rep->last_line_search_k = bestK;
        rep->evaluations = ctx->evaluations;
    }
    return DMSA_OK;
}
// calcNumericJacobian's increment (:199-232)
static double jacobian_increment() { return 1.0 * std::sqrt((double)std::numeric_limits<float>::epsilon()); }


// ---- the host-driven optimizeSet loop (DmsaOptimizer.h:54-150) -------------------------------------------------------------
// What one call of the host-driven loop keeps from iteration to iteration, and the parts of an iteration that enqueue a batch.
struct HostLoop {
    dmsa_ctx* const ctx;
    const dmsa_settings& s;
    const int P;
    // use_analytic_jacobi: the Gaussian rows of J from the pose-table derivatives (analytic_jacobian.h), one evaluation instead of 1 + P
    const bool analytic;
    const double increment = jacobian_increment(), one_div_incr = 1.0 / increment;
    std::vector<double> paramVec, origin, loop, globs, extra;
    HostLmSolve lm;
    HostLoop(dmsa_ctx* c, const dmsa_settings& settings)
        : ctx(c), s(settings), P(num_params(c)), analytic(settings.use_analytic_jacobi != 0), paramVec((size_t)P), origin((size_t)P), loop((size_t)P) {}

    // Host part of evaluation 0 (:99) and of the P forward-difference evaluations of calcNumericJacobian (:199-232):
    // one batch of 1+P pose tables.
    int jacobian_batch() {
        globs.clear(), extra.clear();
        host_eval(ctx, globs, extra);
        chain(ctx).get_params(origin.data());  // :204 (after updateImuError's global2relative round trip)
        auto perturbed = [&](int k, double* out) {
            std::copy(origin.begin(), origin.end(), out);
            out[k] += increment;
        };
        if (ctx->model == MODEL_KEYFRAMES && P >= 48) {
            // the P perturbed chains side by side; the chain is left where the serial loop would leave it: last perturbation evaluated, then
            // (below) parameters restored
            keyframe_chains_aside(ctx, P, P, 1, perturbed, globs, extra, loop);
        } else {
            for (int k = 0; k < P; ++k) {
                perturbed(k, loop.data());
                host_set_params(ctx, loop.data());
                host_eval(ctx, globs, extra);
            }
        }
        chain(ctx).set_params(origin.data());  // :231
        // The tables of the batch (and, on the default path, their transposed copy) depend on nothing the GPU is busy with: they go
        // to another stream, beside the voxelisation, instead of between the fit and the correspondence kernels.
        // On the main stream: the fit launched before and after this point reads table 0 of d_tables, which this batch rewrites (with
        // the same bits) -- in stream order that is no race.  (The device-resident loop keeps the base table in its own buffer and
        // builds the batch beside the voxelisation.)
        hipStream_t ts = ctx->stream;
        // analytic Jacobian: the perturbed chains feed the additional rows only -- evaluation 0 is the one table and the one evaluation
        CHK(build_tables(ctx, analytic ? 1 : 1 + P, globs, ts));
        if (analytic) ctx->evaluations -= P;
        return ctx->tables.signal_owed(ts, ctx->stream);
    }
    // the residuals of the batch (analytic: e0 and the columns of J), then the normal equations
    int residuals_and_normal_equations() {
        if (analytic) {
            CHK(ensure_E(ctx, 1 + P));
            CHK(run_residuals(ctx, 1, nullptr));                          // e0 of the Gaussians
            if (ctx->extra_rows > 0) CHK(upload_extra(ctx, extra, 1 + P));  // the additional rows of all 1 + P parameter sets
            CHK(analytic_columns(ctx, P, one_div_incr, ctx->base_table));
        } else {
            CHK(run_residuals(ctx, 1 + P, &extra));
        }
        const int rowsE = ctx->M + ctx->extra_rows;
        ScopedTimer tm(ctx, T_NORMAL);
        HIPCHK(ctx->d_ne_partial.ensure((size_t)normal_equations_partial_doubles(rowsE, P) * 8));
        HIPCHK(ctx->d_Hp.ensure((size_t)(P + 1) * (P + 1) * 8));
        launch_normal_equations(ctx->d_E.as<double>(), ctx->ldE, rowsE, P, one_div_incr, ctx->d_ne_partial.as<double>(), ctx->d_Hp.as<double>(), ctx->stream,
                                true, nullptr, analytic, ctx->dbg.ne_triangle != 0);
        return DMSA_OK;
    }
};
// :125-128 the step scaled so that its largest element is max_step
static void clamp_step(std::vector<double>& step, double max_step) {
    double mx = -std::numeric_limits<double>::infinity(), mn = std::numeric_limits<double>::infinity();
    for (double v : step) mx = std::max(mx, v), mn = std::min(mn, v);
    const double maxElem = std::max(mx, -mn);  // :125
    if (maxElem > max_step)
        for (double& v : step) v = (max_step / maxElem) * v;
}
static int optimize_host_loop(dmsa_ctx* ctx, const dmsa_settings& s, dmsa_report* rep) {
    ScopedTimer total(ctx, T_TOTAL);
    const bool fixed = (ctx->flags & DMSA_FLAG_FIXED_ITERS) != 0;
    HostLoop h(ctx, s);
    const int P = h.P;
    std::vector<double>& step = h.lm.step;
    int stop = DMSA_STOP_NUM_ITER, iters = 0, bestK = 0;
    double error0 = 0.0, stepNorm = 0.0;
    ctx->evaluations = 0;
    ctx->trace.clear();
    if (h.analytic) CHK(check_analytic_jacobian(ctx, P));

    if (s.use_centralization) CHK(dmsa_centralize(ctx));
    HIPCHK(ctx->d_tables.ensure((size_t)(P + 1) * ctx->rows * 48));  // never reallocated while kernels read it
    for (int iter = 0; iter < s.num_iter; ++iter) {
        ++iters;
        ctx->tl.on = ctx->dbg.host_timeline != 0, ctx->tl.reset(), ctx->tl.mark("start");
        chain(ctx).get_params(h.paramVec.data());  // :72
        // :75 updateGlobalPoints (the window model re-chains here, the keyframe model did in setPoseParameters)
        if (ctx->model == MODEL_WINDOW) chain(ctx).relative_to_global();
        h.globs.clear();
        append_glob(chain(ctx), h.globs);
        CHK(build_tables(ctx, 1, h.globs));
        CHK(transform_points(ctx, 0));
        // the table derivatives at the parameters of the iteration start (before evaluation 0's additional rows touch the chain)
        if (h.analytic) CHK(host_table_derivatives(ctx, ctx->stream));
        ctx->tl.mark("table0+transform enq");
        // The batch does not depend on the Gaussians, so its host math (on the parity path: 1 + P libm pose tables) and the
        // pose-table upload / kernel are issued while the GPU is still voxelising (table 0 of the batch equals the base table the
        // fit reads).  The host-side order of evaluations is the reference's either way; only the early exit below has to undo it.
        const bool overlap = ctx->dbg.overlap_batch != 0;
        const int evals_before = ctx->evaluations;
        const PoseChain chain_before = chain(ctx);  // exact undo, incl. the pose-0 round trip updateImuError leaves behind
        BuildRequest rq;
        if (overlap) rq.overlap = [&h]() { return h.jacobian_batch(); };
        CHK(build_gaussians(ctx, s, rq));  // :78-86, :96
        ctx->tl.mark("build_gaussians (incl. sync#2)");
        ctx->trace.push_back(dmsa_iter_trace{ctx->M, ctx->M1, ctx->Mm, 0.0, 0.0, 0, 0});
        if (ctx->M < s.min_num_gaussians) {  // :89-93
            stop = DMSA_STOP_FEW_GAUSSIANS;
            if (overlap) {  // undo the speculative batch: the reference had not evaluated anything in this iteration
                ctx->evaluations = evals_before;
                chain(ctx) = chain_before;
            }
            break;
        }
        if (!overlap) CHK(h.jacobian_batch());
        CHK(h.residuals_and_normal_equations());
        CHK(h.lm.run(ctx, s, P, ctx->dbg.solve_threads, "sync#3 wait", &error0));  // :101-113
        ctx->tl.mark("assemble+solve");
        bool anyNan = false;
        for (double v : step) anyNan = anyNan || std::isnan(v);
        if (anyNan) {  // :116-122 setPoseParameters(paramVec); break
            chain(ctx).set_params(h.paramVec.data());
            if (ctx->model == MODEL_KEYFRAMES) chain(ctx).relative_to_global();
            stop = DMSA_STOP_NAN;
            break;
        }
        clamp_step(step, s.max_step);
        // adaptiveStepSize (:152-182): nine trial evaluations in one batch
        CHK(host_adaptive_step_size(ctx, P, h.paramVec, step, error0, &bestK));
        double ss = 0.0;
        for (double v : step) ss += v * v;
        stepNorm = std::sqrt(ss);
        ctx->trace.back().error0 = error0, ctx->trace.back().step_norm = stepNorm, ctx->trace.back().best_k = bestK;
        if (bestK == 0 && !fixed) {  // :130-134 — the set is left at raw + 0.9*step (last trial), not restored
            stop = DMSA_STOP_NO_IMPROVEMENT;
            break;
        }
        // :136 setPoseParameters(paramVec): the keyframe model re-chains, the window model only rewrites the relative poses
        chain(ctx).set_params(h.paramVec.data());
        if (ctx->model == MODEL_KEYFRAMES) chain(ctx).relative_to_global();
        if (stepNorm < s.epsilon && !fixed) {  // :139-143
            stop = DMSA_STOP_EPSILON;
            break;
        }
    }
    ctx->tl.print();
    return finish_call(ctx, s, rep, iters, stop, error0, stepNorm, bestK);
}


// ---- the same loop with its control state on the device (loop_kernels.h) ---------------------------------------------------------
// Per iteration the host only enqueues; its one wait is for the Gaussian counts that size the correspondence launches (sync A).  The
// stop decision of iteration i (no improvement / epsilon / NaN step) is taken on the device and reaches the host with the counts of
// iteration i + 1: every loop kernel of a stopped loop is a no-op, so the extra voxelisation that was already enqueued changes nothing.
// The LM step is solved on the device as well (one workgroup up to P = 64, the panel kernel up to P = 1024); only beyond that the
// normal equations go to the host's worker pool, which costs one more wait per iteration.
// The call is a plan (LoopPlan: every mode, decided once by make_loop_plan), its buffers (LoopBuffers) and the phases of a DeviceLoop.

// :107-128 on the device for 64 < P <= 1024: column-block workgroups handing panels to each other, or (lm_stream) a stream of pivot-step records
static int device_lm_panels(dmsa_ctx* ctx, const double* d_Hp, int P, double lambda, double alpha, double max_step, double* d_step, LoopFlags* d_flags, bool lm_stream) {
    const size_t bytes = loop_panel_solve_doubles(P) * 8;
    if (bytes > ctx->d_panel_work.cap || P != ctx->panel_P) {
        // a new size moves the epoch-tagged words (hand-over flags, record counter) onto what used to be data: start from zeros
        HIPCHK(ctx->d_panel_work.ensure(bytes));
        HIPCHK(hipMemsetAsync(ctx->d_panel_work.p, 0, ctx->d_panel_work.cap, ctx->stream));
        ctx->panel_epoch = 0, ctx->panel_P = P;
    }
    const uint32_t epoch = next_epoch(ctx->panel_epoch);
    if (lm_stream && loop_lm_stream_fits(P))
        launch_loop_lm_stream(d_Hp, P, lambda, alpha, max_step, ctx->d_panel_work.as<double>(), epoch, d_step, d_flags, ctx->stream);
    else
        launch_loop_lm_panels(d_Hp, P, lambda, alpha, max_step, ctx->d_panel_work.as<double>(), epoch, d_step, d_flags, ctx->stream);
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}
// :107-128 on the device: one workgroup for P <= 64, the panel solve beyond (also the C ABI's dmsa_lm_solve_device)
int device_lm_step(dmsa_ctx* ctx, const double* d_Hp, int P, double lambda, double alpha, double max_step, double* d_step, LoopFlags* d_flags) {
    if (P > kLoopSolveMaxP) return device_lm_panels(ctx, d_Hp, P, lambda, alpha, max_step, d_step, d_flags, ctx->dbg.lm_stream != 0);
    launch_loop_lm_step(d_Hp, P, lambda, alpha, max_step, d_step, d_flags, ctx->stream);
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}

// ---- The plan: every decision of one call --------------------------------------------------------------------------
enum class LmTier { Partials, Panels, Host };  // who solves :107-128: the one-workgroup kernel on the block sums, the panel kernels, the host's worker pool
struct LoopPlan {
    int P, n, a;  // parameters, poses of the chain, additional rows
    int num_iter;
    int iter_cap;  // iterations the per-iteration buffers are sized for
    bool fixed;
    bool analytic;  // use_analytic_jacobi, see HostLoop
    int skip_mode;  // eval_skip where it applies (0: every pair is computed)
    bool skip_stats;
    int head_mode;  // next_head
    bool head_on;   // the base table of every iteration but the first is adopted from the previous line search
    hipStream_t side;  // the stream of the Jacobian batch's chains and tables, beside the voxelisation
    bool use_rot_same;  // the pose-table kernels flag the evaluations whose rotations are evaluation 0's
    bool rows_aside_allowed;  // the trial chains' IMU rows on the side stream
    bool stamps, per_iter_stamps;  // gap_stamps: the four call-wide slots; the eight slots of every iteration
    LmTier solve;
    bool lm_stream;
    int solve_threads;
    bool one_readback;
    bool ne_triangle;
    bool host_timeline;
    int trace_time;
    double increment, one_div_incr;
};
static LoopPlan make_loop_plan(const dmsa_ctx* ctx, const dmsa_settings& s) {
    const LoopModel& m = ctx->loop_model;
    LoopPlan p{};
    p.P = m.P, p.n = m.n, p.a = m.extra > 0 ? m.extra : 0;
    p.num_iter = std::max(0, s.num_iter);
    // sized for at least 256 iterations from the first call on: a call with more iterations than the one before must not pay a hipMalloc /
    // pinned allocation inside optimizeSet (0.4 ms, seen as 2.5 % of a 20-iteration call that followed a 5-iteration one)
    p.iter_cap = std::max(p.num_iter + 1, 256);
    p.fixed = (ctx->flags & DMSA_FLAG_FIXED_ITERS) != 0;
    p.analytic = s.use_analytic_jacobi != 0;
    p.increment = jacobian_increment(), p.one_div_incr = 1.0 / p.increment;
    p.solve = p.P <= kLoopSolveMaxP ? LmTier::Partials : p.P <= kLoopPanelMaxP ? LmTier::Panels : LmTier::Host;
    p.lm_stream = ctx->dbg.lm_stream != 0, p.solve_threads = ctx->dbg.solve_threads;
    // Pairs (Gaussian, evaluation) whose pose-table rows all have evaluation 0's bits are not computed (serial_kernels.h).  Worth it where
    // a Gaussian's evaluations fill several sub-batches of sixteen lanes, i.e. in the keyframe pass; the one consumer that then has to know
    // is the Jacobian column kernel of the matrix-core normal equations (P > 64).
    p.skip_mode = p.P > kLoopSolveMaxP && !p.analytic ? ctx->dbg.eval_skip : 0;
    p.skip_stats = ctx->dbg.skip_stats != 0 || ctx->dbg.eval_skip == 2;
    p.side = ctx->dbg.dual_stream != 0 ? ctx->stream3 : ctx->stream;
    // Debug switch next_head: from the second iteration of a call on, the base table is not computed.  It is one of the tables the line search
    // of the previous iteration evaluated, or the previous base table: k_loop_finish chains the next iteration from the parameters of the
    // winning trial k (raw + 0.1 k step, the trial chain's expression) or, when no trial won, from the raw parameters, and the global poses are
    // a function of the relative poses alone.  It leaves k in LoopFlags::head_k -- 0 also for a stopped loop and a NaN step, whose control poses
    // did not move -- and k_transform_aabb_adopt reads its table through it and copies it to d_table0 for the fit.  k_window_pose_tables
    // (9.4 us, one workgroup per 256 rows of double math) leaves the head of the iteration; the trial tables get a buffer of their own, because
    // the side stream writes the next Jacobian batch's into d_tables as soon as k_loop_finish is through.
    // Not for windows with IMU rows: updateImuError's global2relative rewrites relative pose 0 in every evaluation, so trial k ran on the pose 0
    // that k - 1 round trips left and the next iteration starts from the one after nine.  Not for keyframe sets (the switch is about the window's
    // interpolated tables), nor with stage timers, whose pose_table_ms is the kernel's time.  Iteration 0 of every call -- the first one
    // behind an upload, a stage call or a restore -- computes its table.  1: from kNextHeadMinPoints on, 2: whatever the size, 3: as 2, IMU
    // windows included, and the table is also computed the present way and compared (dmsa_debug_next_head).
    constexpr int64_t kNextHeadMinPoints = 0;  // (no kernel is added and one leaves: profiles/r18_next_head_ab.txt has the smallest windows)
    p.head_mode = ctx->dbg.next_head;
    p.head_on = p.head_mode != 0 && ctx->model == MODEL_WINDOW && ctx->n > 0 && (ctx->flags & DMSA_FLAG_STAGE_TIMERS) == 0 && (p.a == 0 || p.head_mode == 3) &&
                (p.head_mode >= 2 || ctx->n >= kNextHeadMinPoints);
    // with the flags that let the correspondence kernels share the rotated coordinates among the translation differences (serial_kernels.hip)
    p.use_rot_same = ctx->dbg.shared_rotations != 0 && !p.analytic;
    // A window with IMU rows: the rows (updateImuError: a dozen Floater-Hormann evaluations per row) are half of the chain kernel's time and nobody
    // reads them before the squared sums -- the main stream computes the control poses only (part 1), the side stream the rows and the state the
    // last trial leaves (part 2) beside the pose tables and the trial batch.  26 + 4 us -> 11 us in front of the trial batch of a config-2 window.
    // (by_counter follows dbg.device_sync, which only optimize() changes, and only between two runs of a call: constant inside one run, so the
    // rule is the plan's.)
    p.rows_aside_allowed = ctx->dbg.trial_rows_aside != 0 && p.a > 0 && ctx->model == MODEL_WINDOW && ctx->trial_step.by_counter() && p.side != ctx->stream;
    // debug switch gap_stamps: one-thread kernels write the device's wall clock; 2 = eight stamps per iteration, printed as a table
    p.stamps = ctx->dbg.gap_stamps != 0, p.per_iter_stamps = ctx->dbg.gap_stamps >= 2;
    p.one_readback = ctx->dbg.one_readback != 0;
    p.ne_triangle = ctx->dbg.ne_triangle != 0;
    p.host_timeline = ctx->dbg.host_timeline != 0;
    p.trace_time = ctx->dbg.trace_time;  // where a call's time outside its iterations goes (host clock, microseconds since the call began)
    return p;
}

// ---- The buffers of one call: every size, every carved pointer ---------------------------------------------------------
struct LoopBuffers {
    size_t st;  // doubles of one chain state
    double *S0, *S1, *S2;  // chain states: start of the iteration, after the Jacobian batch, after the line search
    double *d_param, *d_step;
    double *d_extra_jac, *d_extra_trial;  // additional rows of the two batches
    double* d_error0;  // e0^T e0, element (P, P) of Hp
    LoopFlags* d_flags;
    IterResult *d_results, *h_results;
    uint32_t* rot_same;  // (null: not shared)
    long long *call_stamps, *iter_stamps;  // gap_stamps (null: off)
    bool head_mismatches_fresh;  // d_head_mismatches was allocated by this call: seed() zeroes it
};
static int make_loop_buffers(dmsa_ctx* ctx, const LoopPlan& p, LoopBuffers* out) {
    const int P = p.P, n = p.n, a = p.a;
    LoopBuffers b{};
    b.st = loop_state_doubles(n);
    if (p.analytic) {
        HIPCHK(ctx->d_ctrl_pm.ensure(2 * (size_t)P * n * 6 * 8));
        HIPCHK(ctx->d_dT.ensure((size_t)ctx->rows * 12 * P * 8));
    }
    HIPCHK(ctx->d_loop_state.ensure(3 * b.st * 8));
    HIPCHK(ctx->d_loop_vec.ensure((size_t)2 * P * 8 + 64));
    HIPCHK(ctx->d_ctrl0.ensure((size_t)n * 6 * 8));
    HIPCHK(ctx->d_ctrl.ensure((size_t)(1 + P) * n * 6 * 8));
    HIPCHK(ctx->d_table0.ensure((size_t)ctx->rows * 48));
    HIPCHK(ctx->d_tables.ensure((size_t)(P + 1) * ctx->rows * 48));  // never reallocated while kernels read it
    HIPCHK(ctx->d_tablesT.ensure((size_t)(P + 1) * ctx->rows * 48));
    HIPCHK(ctx->d_loop_extra.ensure((size_t)(1 + P + 9) * std::max(a, 1) * 8));
    HIPCHK(ctx->d_rot_same.ensure((size_t)(1 + P) * 4));
    if (p.skip_mode != 0) {
        HIPCHK(ctx->d_row_range.ensure((size_t)(1 + P) * 8));
        if ((size_t)P * 16 > ctx->d_skip_stats.cap) {  // per evaluation: pairs left out, pairs that differed under eval_skip = 2
            HIPCHK(ctx->d_skip_stats.ensure((size_t)P * 16));
            HIPCHK(hipMemsetAsync(ctx->d_skip_stats.p, 0, ctx->d_skip_stats.cap, ctx->stream));
            ctx->skip_stats_evals = P;
        }
    }
    HIPCHK(ctx->d_loop_iter.ensure(sizeof(LoopFlags) + (size_t)p.iter_cap * sizeof(IterResult)));
    HIPCHK(ctx->d_Hp.ensure((size_t)(P + 1) * (P + 1) * 8));
    HIPCHK(ctx->d_sq_out.ensure(16 * 8));
    HIPCHK(ctx->h_results.ensure((size_t)(p.num_iter + 1) * sizeof(IterResult), nullptr /* every call ends with a host wait */, (size_t)(p.iter_cap + 16) * sizeof(IterResult)));
    if (p.stamps) {
        HIPCHK(ctx->d_gap_stamps.ensure((size_t)(16 + 8 * (p.per_iter_stamps ? p.num_iter : 0)) * 8));
        b.call_stamps = ctx->d_gap_stamps.as<long long>();
        if (p.per_iter_stamps) b.iter_stamps = b.call_stamps + 16;
    }
    if (p.head_on) {
        HIPCHK(ctx->d_trial_tables.ensure((size_t)9 * ctx->rows * 48));
        if (p.head_mode == 3) {
            HIPCHK(ctx->d_head_check.ensure((size_t)ctx->rows * 48));
            if (ctx->d_head_mismatches.p == nullptr) {
                HIPCHK(ctx->d_head_mismatches.ensure(8));
                b.head_mismatches_fresh = true;
            }
        }
    }
    b.h_results = ctx->h_results.as<IterResult>();
    std::memset(b.h_results, 0, (size_t)(p.num_iter + 1) * sizeof(IterResult));
    b.S0 = ctx->d_loop_state.as<double>(), b.S1 = b.S0 + b.st, b.S2 = b.S1 + b.st;
    b.d_param = ctx->d_loop_vec.as<double>(), b.d_step = b.d_param + P;
    b.d_extra_jac = ctx->d_loop_extra.as<double>(), b.d_extra_trial = b.d_extra_jac + (size_t)(1 + P) * a;
    b.d_error0 = ctx->d_Hp.as<double>() + (size_t)P * (P + 1) + P;
    b.d_flags = ctx->d_loop_iter.as<LoopFlags>();
    b.d_results = reinterpret_cast<IterResult*>(b.d_flags + 1);
    b.rot_same = p.use_rot_same ? ctx->d_rot_same.as<uint32_t>() : nullptr;
    *out = b;
    return DMSA_OK;
}

// the per-iteration slots of gap_stamps = 2 (1 and 2 are build_gaussians', through ctx->stamp_voxel / stamp_fit); slots 3 .. 6 are also the four
// call-wide slots of gap_stamps = 1, which keep the last iteration's
enum StampSlot { STAMP_BEGIN = 0, STAMP_VOXEL, STAMP_FIT, STAMP_JACOBIAN, STAMP_NORMAL, STAMP_LM, STAMP_TRIALS, STAMP_END };
static int gap_stamps_print(dmsa_ctx* ctx, const LoopBuffers& b, int iters, int P) {
    if (b.iter_stamps && iters > 0) {
        std::vector<long long> t((size_t)8 * iters);
        HIPCHK(hipMemcpy(t.data(), b.iter_stamps, t.size() * 8, hipMemcpyDeviceToHost));
        std::fprintf(stderr, "[gap_stamps] per iteration, us on the device's wall clock (each stamp kernel adds ~3 us): voxelisation | fit | Jacobian batch | normal equations | LM step | "
                             "trial chains + tables | trial batch + decision | whole iteration\n");
        for (int i = 0; i < iters; ++i) {
            const long long* r = t.data() + 8 * i;
            std::fprintf(stderr, "[gap_stamps] %3d:", i);
            for (int k = 1; k < 8; ++k) std::fprintf(stderr, " %6.1f", (r[k] - r[k - 1]) * 0.01);
            std::fprintf(stderr, " | %6.1f\n", i + 1 < iters ? (t[(size_t)8 * (i + 1)] - r[0]) * 0.01 : (r[7] - r[0]) * 0.01);
        }
    }
    if (b.call_stamps && iters > 0) {
        long long t[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpy(t, b.call_stamps, sizeof(t), hipMemcpyDeviceToHost));
        std::fprintf(stderr, "[gap_stamps] last iteration, P = %d, %d rows: Jacobian batch joined -> normal equations done %.1f us -> LM step done %.1f us -> trial chains + tables done %.1f us "
                             "(device wall clock, unprofiled; each stamp kernel adds its own ~3 us)\n", P, ctx->M + ctx->extra_rows, (t[1] - t[0]) * 0.01, (t[2] - t[1]) * 0.01, (t[3] - t[2]) * 0.01);
    }
    return DMSA_OK;
}

// ---- One call: the phases ------------------------------------------------------------------------------------------
// Each phase enqueues what its name says, on the streams the plan names, and decides no mode.  What one phase leaves for a later one (the
// rows of E, a NaN the host's solve saw) is a member below the plan.
struct DeviceLoop {
    dmsa_ctx* const ctx;
    const dmsa_settings& s;
    const LoopPlan& p;
    const LoopBuffers& b;
    const LoopModel& m;
    const std::chrono::steady_clock::time_point call_t0;  // trace_time
    std::string call_trace;
    BuildRequest rq;  // side_head: side_batch, for every voxelisation of the call
    HostLmSolve lm;   // P > kLoopPanelMaxP only
    int iters = 0, stop = DMSA_STOP_NUM_ITER;
    // what the report says about the Gaussians belongs to the last iteration that really ran
    int last_M = 0, last_M1 = 0;
    int64_t last_Mm = 0;
    int nan_evals = 0;
    int rowsE = 0;          // rows of E in this iteration's batches
    bool host_nan = false;  // the host's solve (LmTier::Host) saw a NaN step
    double error0 = 0.0, stepNorm = 0.0;  // fold_results
    int bestK = 0;

    DeviceLoop(dmsa_ctx* c, const dmsa_settings& settings, const LoopPlan& plan, const LoopBuffers& buffers, std::chrono::steady_clock::time_point t0)
        : ctx(c), s(settings), p(plan), b(buffers), m(c->loop_model), call_t0(t0) {
        rq.side_head = [this]() { return side_batch(); };
    }
    DeviceLoop(const DeviceLoop&) = delete;
    DeviceLoop& operator=(const DeviceLoop&) = delete;

    void mark(const char* what) {
        if (p.trace_time == 0) return;
        char buf[160];
        std::snprintf(buf, sizeof(buf), " %s %.0f", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - call_t0).count());
        call_trace += buf;
    }
    // the wall clock of the device at this point of the main stream, into whichever stamp family has the slot
    void stamp(int iter, int slot) {
        if (p.stamps && slot >= STAMP_JACOBIAN && slot <= STAMP_TRIALS) launch_stamp(b.call_stamps + (slot - STAMP_JACOBIAN), ctx->stream);
        if (p.per_iter_stamps) launch_stamp(b.iter_stamps + 8 * iter + slot, ctx->stream);
    }

    // the host chain as centralize() left it, cleared flags and results; then the zeros of the stamps and of a new mismatch counter
    int seed() {
        PoseChain& c = chain(ctx);
        const int n = p.n;
        double* pin = nullptr;
        CHK(pinned_doubles(ctx, b.st, &pin));
        std::copy(c.rel_o.begin(), c.rel_o.end(), pin);
        std::copy(c.rel_t.begin(), c.rel_t.end(), pin + 3 * n);
        std::copy(c.glob_o.begin(), c.glob_o.end(), pin + 6 * n);
        std::copy(c.glob_t.begin(), c.glob_t.end(), pin + 9 * n);
        HIPCHK(hipMemcpyAsync(b.S0, pin, b.st * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemsetAsync(ctx->d_loop_iter.p, 0, sizeof(LoopFlags) + (size_t)(p.num_iter + 1) * sizeof(IterResult), ctx->stream));
        mark("seeded");
        if (p.per_iter_stamps) HIPCHK(hipMemsetAsync(b.iter_stamps, 0, (size_t)8 * p.num_iter * 8, ctx->stream));
        if (b.head_mismatches_fresh) HIPCHK(hipMemsetAsync(ctx->d_head_mismatches.p, 0, 8, ctx->stream));
        return DMSA_OK;
    }

    // :72-75 parameters, chain, base table, global points
    int head(int iter) {
        ctx->tl.on = p.host_timeline, ctx->tl.reset(), ctx->tl.mark("start");
        // the Jacobian chains on the side stream start when the state of the iteration start is in place: signalled by k_loop_begin /
        // the previous k_loop_finish themselves (dev_sync.h) -- no event on the main stream
        stamp(iter, STAMP_BEGIN);  // the iteration begins
        if (p.per_iter_stamps) ctx->stamp_voxel = b.iter_stamps + 8 * iter + STAMP_VOXEL, ctx->stamp_fit = b.iter_stamps + 8 * iter + STAMP_FIT;
        if (iter == 0)  // later iterations: done by loop_finish
            launch_loop_begin(m, b.S0, b.d_param, ctx->d_ctrl0.as<double>(), b.d_flags, ctx->stream, ctx->loop_state.kernel_signal(ctx->stream, p.side));
        const bool adopt = p.head_on && iter > 0;  // the previous iteration of this call left its trial tables and its decision
        if (!adopt) {
            ScopedTimer tm(ctx, T_TABLE);
            CHK(device_tables(ctx, 1, ctx->d_ctrl0.as<double>(), ctx->d_table0.as<float>(), nullptr, ctx->stream));
        }
        ctx->base_table = ctx->d_table0.as<float>();
        if (adopt) {
            ScopedTimer tm(ctx, T_VOXEL);
            launch_transform_aabb_adopt(ctx->d_local.as<float4>(), ctx->d_table0.as<float4>(), ctx->d_trial_tables.as<float4>(), ctx->rows, &b.d_flags->head_k,
                                        ctx->d_global.as<float4>(), ctx->n, ctx->d_aabb.as<float>(), ctx->d_counts.p, sizeof(GaussCounts) + sizeof(SerialCounts),
                                        ctx->stream);
            ctx->aabb_fresh = true;
            ctx->next_head_iterations += 1;
            if (p.head_mode == 3) {  // the present kernel on the same control poses, and a comparison: two more kernels on the main stream
                CHK(device_tables(ctx, 1, ctx->d_ctrl0.as<double>(), ctx->d_head_check.as<float>(), nullptr, ctx->stream));
                launch_count_word_mismatches(ctx->d_table0.p, ctx->d_head_check.p, ctx->rows * 12, ctx->d_head_mismatches.as<unsigned long long>(), ctx->stream);
            }
        } else {
            ScopedTimer tm(ctx, T_VOXEL);
            launch_transform_aabb(ctx->d_local.as<float4>(), ctx->model == MODEL_KEYFRAMES ? ctx->d_nlocal.as<float4>() : nullptr, ctx->d_table0.as<float4>(),
                                  ctx->d_global.as<float4>(), ctx->model == MODEL_KEYFRAMES ? ctx->d_nglobal.as<float4>() : nullptr, ctx->n,
                                  ctx->d_aabb.as<float>(), ctx->d_counts.p, sizeof(GaussCounts) + sizeof(SerialCounts), ctx->stream);
            ctx->aabb_fresh = true;
        }
        if (!ctx->loop_state.by_counter()) CHK(ctx->loop_state.signal(ctx->stream, p.side));  // (events: recorded here, behind the transform)
        ctx->tl.mark("begin+batch enq");
        return DMSA_OK;
    }

    // :99, :199-232 the 1 + P chains, rows and pose tables of the Jacobian batch: beside the voxelisation, they need nothing from it.
    // build_gaussians enqueues them (its side_head): first of all, or behind the k_lattice it puts on the side stream (debug switch keys_ahead).
    int side_batch() {
        const int P = p.P;
        hipStream_t side = p.side;
        CHK(ctx->loop_state.wait(side, ctx->stream));
        launch_loop_chain(m, 0, b.S0, b.S1, b.d_param, b.d_step, p.increment, ctx->d_ctrl.as<double>(), b.d_extra_jac, b.d_flags, side);
        if (p.analytic) {
            // evaluation 0's table, and the table derivatives from the 2P central-difference chains of the iteration start
            launch_loop_chain_central(m, b.S0, kTableDerivStep, ctx->d_ctrl_pm.as<double>(), b.d_flags, side);
            CHK(table_derivatives(ctx, ctx->d_ctrl_pm.as<double>(), side));
            CHK(device_tables(ctx, 1, ctx->d_ctrl.as<double>(), ctx->d_tables.as<float>(), ctx->d_tablesT.as<float>(), side));
            ctx->batch = 1, ctx->tablesT_batch = 1;
        } else {
            CHK(device_tables(ctx, 1 + P, ctx->d_ctrl.as<double>(), ctx->d_tables.as<float>(), ctx->d_tablesT.as<float>(), side, b.rot_same));
            ctx->batch = 1 + P, ctx->tablesT_batch = 1 + P;
        }
        if (p.skip_mode != 0)
            launch_eval_row_ranges(m.model, ctx->d_ctrl.as<double>(), 1 + P, p.n, ctx->d_stamps.as<double>(), ctx->d_trajtime.as<double>(), ctx->rows - 1,
                                   ctx->d_row_range.as<int2>(), side);
        // the main stream picks the tables up in k_size_classes (or, with events or if that kernel is not launched, in run_residuals)
        return ctx->tables.signal_owed(side, ctx->stream);
    }

    // :78-96; the previous iteration's result rides on the read-back of the counts.  *go_on = false: the loop is over (it ended in the
    // previous iteration, or this one has too few Gaussians)
    int voxelise(int iter, bool* go_on) {
        *go_on = false;
        // (one_readback: k_loop_finish left it in d_readback as well, which the one copy brings over whole; h_results gets it below)
        if (iter > 0 && !p.one_readback) {
            ctx->rb_extra_src = b.d_results + (iter - 1), ctx->rb_extra_dst = b.h_results + (iter - 1), ctx->rb_extra_bytes = sizeof(IterResult);
        } else {
            ctx->rb_extra_bytes = 0;
        }
        const int rc = build_gaussians(ctx, s, rq);
        ctx->rb_extra_bytes = 0;
        CHK(rc);
        if (iter > 0 && p.one_readback) b.h_results[iter - 1] = ctx->rb()->prev;
        drain_timers(ctx);  // everything the previous iteration timed has completed
        ctx->tl.mark("build_gaussians (incl. sync A)");
        if (iter == 0) mark("first-counts");
        if (iter == 1) mark("second-counts");
        if (iter > 1 && p.trace_time >= 2) {  // every iteration's: the host's iteration period is the device's
            char what[96];
            std::snprintf(what, sizeof(what), "[M %d Mm %lld grown %lld] counts", ctx->M, (long long)ctx->Mm, DevBuf::reallocations());
            mark(what);
        }
        if (iter > 0 && b.h_results[iter - 1].stop != 0) return DMSA_OK;  // the loop ended in the previous iteration: this one never started
        ++iters;
        last_M = ctx->M, last_M1 = ctx->M1, last_Mm = ctx->Mm;
        ctx->trace.push_back(dmsa_iter_trace{ctx->M, ctx->M1, ctx->Mm, 0.0, 0.0, 0, 0});
        if (ctx->M < s.min_num_gaussians) {  // :89-93 -- nothing of this iteration has touched the state the next call starts from (S0)
            stop = DMSA_STOP_FEW_GAUSSIANS;
            return DMSA_OK;
        }
        *go_on = true;
        return DMSA_OK;
    }

    // the residuals of the 1 + P evaluations (analytic: e0, then the columns of J) on the tier streams
    int jacobian_batch(int iter) {
        const int P = p.P;
        if (p.analytic) {
            ctx->evaluations += 1;
            CHK(ensure_E(ctx, 1 + P));
            CHK(run_residuals(ctx, 1, nullptr));  // e0 of the Gaussians
            if (p.a > 0) launch_loop_scatter_extra(b.d_extra_jac, 1 + P, p.a, ctx->d_E.as<double>(), ctx->ldE, ctx->M, ctx->stream);
            CHK(analytic_columns(ctx, P, p.one_div_incr, ctx->d_table0.as<float>()));
        } else {
            ctx->evaluations += 1 + P;
            if (p.skip_mode != 0) ctx->skip_pairs += (int64_t)ctx->M * P;
            CHK(run_residuals(ctx, 1 + P, nullptr, b.d_extra_jac, b.rot_same, p.skip_mode == 1 ? ctx->d_row_range.as<int2>() : nullptr));
        }
        rowsE = ctx->M + ctx->extra_rows;
        stamp(iter, STAMP_JACOBIAN);  // the Jacobian batch has joined
        return DMSA_OK;
    }

    int normal_equations(int iter) {
        const int P = p.P;
        {
            ScopedTimer tm(ctx, T_NORMAL);
            HIPCHK(ctx->d_ne_partial.ensure((size_t)normal_equations_partial_doubles(rowsE, P) * 8));
            EvalSkip skip;
            if (p.skip_mode != 0)
                skip.row_range = ctx->d_row_range.as<int2>(), skip.gauss_rows = ctx->d_gauss_rows.as<int2>(), skip.M = ctx->M, skip.check = p.skip_mode == 2 ? 1 : 0,
                skip.stats = p.skip_stats ? ctx->d_skip_stats.as<unsigned long long>() : nullptr;
            // P <= 64: the block sums stay unreduced, the solve kernel adds them while it loads the matrix
            launch_normal_equations(ctx->d_E.as<double>(), ctx->ldE, rowsE, P, p.one_div_incr, ctx->d_ne_partial.as<double>(), ctx->d_Hp.as<double>(), ctx->stream,
                                    p.solve != LmTier::Partials, p.skip_mode != 0 ? &skip : nullptr, p.analytic, p.ne_triangle);
        }
        stamp(iter, STAMP_NORMAL);  // normal equations done
        return DMSA_OK;
    }

    // :107-128 the LM step, by the plan's tier
    int lm_step(int iter) {
        const int P = p.P;
        host_nan = false;
        if (p.solve == LmTier::Partials) {
            const NormalEqPartials q = normal_equations_partials(rowsE, P);
            launch_loop_lm_step_partials(ctx->d_ne_partial.as<double>(), q.nsplit, q.nt, P, (double)s.lambda_diag, s.step_length_optim, s.max_step, b.d_step, b.d_flags,
                                         b.d_error0, ctx->stream, p.ne_triangle);
        } else if (p.solve == LmTier::Panels) {
            CHK(device_lm_panels(ctx, ctx->d_Hp.as<double>(), P, (double)s.lambda_diag, s.step_length_optim, s.max_step, b.d_step, b.d_flags, p.lm_stream));
        } else {
            double e0 = 0.0;  // (the device reads its own copy, d_error0)
            CHK(lm.run(ctx, s, P, p.solve_threads, "sync B wait", &e0));  // :107-113
            for (double v : lm.step) host_nan = host_nan || std::isnan(v);
            double* pin = nullptr;
            CHK(pinned_doubles(ctx, (size_t)P, &pin));
            std::memcpy(pin, lm.step.data(), (size_t)P * 8);
            HIPCHK(hipMemcpyAsync(b.d_step, pin, (size_t)P * 8, hipMemcpyHostToDevice, ctx->stream));
            launch_loop_step_finish(P, s.max_step, b.d_step, b.d_flags, ctx->stream);  // NaN test, clamp
            ctx->tl.mark("solve");
        }
        stamp(iter, STAMP_LM);  // LM step done
        return DMSA_OK;
    }

    // :152-182 the chains of the nine trials; with rows aside (the plan's rule) the main stream computes the control poses only
    int trial_chains() {
        if (p.rows_aside_allowed) {
            CHK(ensure_E(ctx, 9));  // (the scatter below needs ldE; the Jacobian batch's E is at least as large)
            launch_loop_chain(m, 1, b.S1, b.S2, b.d_param, b.d_step, p.increment, ctx->d_ctrl.as<double>(), b.d_extra_trial, b.d_flags, ctx->stream, 1,
                              ctx->trial_step.kernel_signal(ctx->stream, p.side));
            CHK(ctx->trial_step.wait(p.side, ctx->stream));
            launch_loop_chain(m, 1, b.S1, b.S2, b.d_param, b.d_step, p.increment, ctx->d_ctrl.as<double>(), b.d_extra_trial, b.d_flags, p.side, 2);
            launch_loop_scatter_extra(b.d_extra_trial, 9, p.a, ctx->d_E.as<double>(), ctx->ldE, ctx->M, p.side);
            CHK(ctx->trial_rows.signal(p.side, ctx->stream));
        } else {
            launch_loop_chain(m, 1, b.S1, b.S2, b.d_param, b.d_step, p.increment, ctx->d_ctrl.as<double>(), b.d_extra_trial, b.d_flags, ctx->stream);
        }
        return DMSA_OK;
    }

    // the nine pose tables, the trial batch, its squared sums and :130-143 the decision (k_loop_finish)
    int trial_batch_and_decision(int iter) {
        const int P = p.P;
        {
            ScopedTimer tm(ctx, T_TABLE);
            // (the correspondence kernels read the transposed tables; the row-major ones are the next iteration's to adopt)
            CHK(device_tables(ctx, 9, ctx->d_ctrl.as<double>(), p.head_on ? ctx->d_trial_tables.as<float>() : ctx->d_tables.as<float>(), ctx->d_tablesT.as<float>(),
                              ctx->stream));
            ctx->batch = 9, ctx->tablesT_batch = 9;
        }
        stamp(iter, STAMP_TRIALS);  // trial chains and pose tables done
        if (!host_nan) ctx->evaluations += 9;
        nan_evals = host_nan ? 0 : 9;
        CHK(run_residuals(ctx, 9, nullptr, p.rows_aside_allowed ? nullptr : b.d_extra_trial));
        {
            ScopedTimer tm(ctx, T_NORMAL);
            HIPCHK(ctx->d_sq_partial.ensure((size_t)squared_sums_blocked_partial_doubles(rowsE, P, 9) * 8));
            DevSync rows_in;  // the side stream's rows: waited for by the kernel that reads them (a one-wave wait kernel in front of it costs 3 us)
            if (p.rows_aside_allowed) ctx->trial_rows.kernel_wait(rows_in);
            launch_squared_sums_blocked(ctx->d_E.as<double>(), ctx->ldE, rowsE, P, 9, ctx->d_sq_partial.as<double>(), nullptr, ctx->stream,
                                        p.rows_aside_allowed ? &rows_in : nullptr);  // block sums only
        }
        // with the signal for the next iteration's chains, if there is one (a signal nobody waits for is harmless)
        launch_loop_finish(m, b.S1, b.S2, b.S0, b.d_param, b.d_step, b.d_error0, ctx->d_sq_partial.as<double>(), normal_equations_partials(rowsE, P).nsplit,
                           p.fixed ? 1 : 0, s.epsilon, b.d_results + iter, b.d_flags, ctx->d_ctrl0.as<double>(), iter + 1 < p.num_iter ? 1 : 0, ctx->stream,
                           ctx->loop_state.kernel_signal(ctx->stream, p.side), p.one_readback ? ctx->d_prev_result() : nullptr);
        stamp(iter, STAMP_END);  // the iteration's last kernel (k_loop_finish) is done
        HIPCHK(hipGetLastError());
        ctx->tl.mark("iteration enq");
        return DMSA_OK;
    }

    // final state and the results not yet seen, back to the host chain and h_results
    int collect() {
        const int n = p.n;
        double* fin = nullptr;
        CHK(pinned_doubles(ctx, b.st, &fin));
        HIPCHK(hipMemcpyAsync(fin, b.S0, b.st * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (iters > 0) HIPCHK(hipMemcpyAsync(b.h_results, b.d_results, (size_t)iters * sizeof(IterResult), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(enqueue_batch_ticks(ctx));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        mark("state-back");
        drain_timers(ctx);
        ctx->stamp_voxel = ctx->stamp_fit = nullptr;
        CHK(gap_stamps_print(ctx, b, iters, p.P));
        PoseChain& c = chain(ctx);  // (nothing has taken a slot of the pinned ring since)
        std::copy(fin, fin + 3 * n, c.rel_o.begin());
        std::copy(fin + 3 * n, fin + 6 * n, c.rel_t.begin());
        std::copy(fin + 6 * n, fin + 9 * n, c.glob_o.begin());
        std::copy(fin + 9 * n, fin + 12 * n, c.glob_t.begin());
        return DMSA_OK;
    }
    // the per-iteration results into the trace and the figures of the report
    void fold_results() {
        for (int i = 0; i < iters && i < (int)ctx->trace.size(); ++i) {
            const IterResult& r = b.h_results[i];
            const bool ran = !(stop == DMSA_STOP_FEW_GAUSSIANS && i == iters - 1);  // the aborted iteration has no step
            if (!ran) break;
            error0 = r.error0;
            if (r.stop == DMSA_STOP_NAN) {  // :116-122: left before the line search, nothing else of this iteration is recorded
                stop = r.stop;
                ctx->evaluations -= nan_evals;
                break;
            }
            ctx->trace[(size_t)i].error0 = r.error0, ctx->trace[(size_t)i].step_norm = r.step_norm, ctx->trace[(size_t)i].best_k = r.best_k;
            stepNorm = r.step_norm, bestK = r.best_k;
            if (r.stop != 0) stop = r.stop;
        }
        ctx->M = last_M, ctx->M1 = last_M1, ctx->Mm = last_Mm;
    }
};

static int optimize_device_loop(dmsa_ctx* ctx, const dmsa_settings& s, dmsa_report* rep) {
    ScopedTimer total(ctx, T_TOTAL);
    const auto call_t0 = std::chrono::steady_clock::now();
    const LoopPlan plan = make_loop_plan(ctx, s);
    ctx->evaluations = 0;
    ctx->trace.clear();
    if (plan.analytic) CHK(check_analytic_jacobian(ctx, plan.P));
    if (s.use_centralization) CHK(dmsa_centralize(ctx));
    LoopBuffers buffers;
    CHK(make_loop_buffers(ctx, plan, &buffers));
    DeviceLoop loop(ctx, s, plan, buffers, call_t0);
    CHK(loop.seed());
    for (int iter = 0; iter < plan.num_iter; ++iter) {
        bool go_on = false;
        CHK(loop.head(iter));
        CHK(loop.voxelise(iter, &go_on));  // (side_batch: enqueued from inside build_gaussians)
        if (!go_on) break;
        CHK(loop.jacobian_batch(iter));
        CHK(loop.normal_equations(iter));
        CHK(loop.lm_step(iter));
        CHK(loop.trial_chains());
        CHK(loop.trial_batch_and_decision(iter));
        if (loop.host_nan) break;  // the device takes the same decision; nothing more to enqueue
    }
    ctx->tl.print();
    loop.mark("all-enqueued");
    CHK(loop.collect());
    loop.fold_results();
    CHK(finish_call(ctx, s, rep, loop.iters, loop.stop, loop.error0, loop.stepNorm, loop.bestK));
    loop.mark("final-points");
    if (plan.trace_time != 0) std::fprintf(stderr, "[call] %d iterations, us since the call began:%s\n", loop.iters, loop.call_trace.c_str());
    return DMSA_OK;
}


// ---- optimize(): one whole optimizeSet call ------------------------------------------------------------------------------
// What a whole call may have to start over from (a device-side wait that gave up means a consumer ran before its producers: nothing of
// that run can be trusted): the host model state, and the static points as they were -- centralize / decentralize shifts them in float
// and is no exact round trip, so a second run on the shifted-back points would not be the run the caller asked for.
struct CallSnapshot {
    bool taken = false;
    WindowHost win;
    KeyframeHost key;
    bool centralized = false;
};
static int take_snapshot(dmsa_ctx* ctx, const dmsa_settings& s, CallSnapshot& snap) {
    snap.win = ctx->win, snap.key = ctx->key, snap.centralized = ctx->centralized;
    if (ctx->model == MODEL_WINDOW && s.use_centralization && ctx->S > 0) {
        HIPCHK(ctx->d_static_keep.ensure((size_t)ctx->S * 16));
        HIPCHK(hipMemcpyAsync(ctx->d_static_keep.p, ctx->d_local.as<float4>() + ctx->N, (size_t)ctx->S * 16, hipMemcpyDeviceToDevice, ctx->stream));
    }
    snap.taken = true;
    return DMSA_OK;
}
static int restore_snapshot(dmsa_ctx* ctx, const dmsa_settings& s, const CallSnapshot& snap) {
    ctx->win = snap.win, ctx->key = snap.key, ctx->centralized = snap.centralized;
    if (ctx->model == MODEL_WINDOW && s.use_centralization && ctx->S > 0) {
        HIPCHK(hipMemcpyAsync(ctx->d_local.as<float4>() + ctx->N, ctx->d_static_keep.p, (size_t)ctx->S * 16, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    ctx->gaussians_valid = false, ctx->order_valid = false, ctx->aabb_fresh = false;
    return DMSA_OK;
}
int optimize(dmsa_ctx* ctx, const dmsa_settings& s, dmsa_report* rep) {
    // the loop state lives on the device (one host wait per iteration); the host-driven loop remains for host-built pose tables, for the
    // debug switch device_loop = 0 and for sets whose chain state does not fit the chain kernels' LDS (hundreds of keyframes)
    const bool device_loop = !(ctx->flags & DMSA_FLAG_POSE_TABLE_HOST) && ctx->dbg.device_loop != 0 && loop_chain_fits(ctx->loop_model);
    auto run = [&]() {
        ctx->wait_seq = 0, ctx->voxel_calls = 0;
        int rc = device_loop ? optimize_device_loop(ctx, s, rep) : optimize_host_loop(ctx, s, rep);
        // A failure inside the loop (HIP error, lattice deeper than 21 levels, allocation) must not leave the resident problem in the centred
        // frame: the static points were shifted in place and the window origin lives only in the context.
        if (rc != DMSA_OK && ctx->centralized) {
            const std::string err = ctx->err;
            (void)dmsa_decentralize(ctx);
            ctx->err = err;
        }
        return rc;
    };
    CallSnapshot snap;
    if (ctx->dbg.device_sync != 0) CHK(take_snapshot(ctx, s, snap));
    int rc = run();
    // The flag is looked at on EVERY exit: a call that failed for another reason after a wait gave up (or after a signal was counted but
    // never enqueued) would otherwise hand a stale flag and mismatched targets to the next, healthy call.
    std::string what;
    if (ctx->dbg.device_sync != 0 && sync_wait_timed_out(ctx, &what)) {
        // Counters in device memory need the producer's queue to make progress while the consumer's wait spins; a tool that serialises
        // kernels across queues in an order of its own (hardware counter collection) breaks that.  The call is run again from the state it
        // started from with event dependencies, and the context keeps them from now on.
        const std::string first = rc == DMSA_OK ? std::string() : " (first attempt: " + ctx->err + ")";
        ctx->dbg.device_sync = 0;
        ctx->sync_retries += 1;
        CHK(restore_snapshot(ctx, s, snap));
        rc = run();
        const std::string warn = "warning: a device-side stream dependency timed out (" + what + "); the call was run again with event dependencies, which this context "
                                 "uses from now on (DMSA_DEBUG=device_sync=0 selects them from the start)" + first;
        ctx->err = rc == DMSA_OK ? warn : ctx->err + " | " + warn;
    }
    return rc;
}
