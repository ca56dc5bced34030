// context.cpp — lifetime of a dmsa_ctx: creation (debug switches), destruction, device buffers, timers; the two flat upload entries (upload_driver.cpp).
#include "dmsa_ctx.h"

#include <cstddef>

WorkerPool& workers(dmsa_ctx* ctx) {
    if (!ctx->pool) {
        const unsigned want = (unsigned)std::max(1, ctx->dbg.host_threads);  // host pose tables, perturbed keyframe chains, upload packing, host solve
        ctx->pool = new WorkerPool((int)std::min(want, std::max(2u, std::thread::hardware_concurrency())));
    }
    return *ctx->pool;
}
hipEvent_t get_event(dmsa_ctx* ctx) {
    if (!ctx->free_events.empty()) {
        hipEvent_t e = ctx->free_events.back();
        ctx->free_events.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
// fold finished event pairs into the accumulators (call after a stream synchronisation)
void drain_timers(dmsa_ctx* ctx) {
    // pairs whose closing event has not completed yet stay pending (the device-resident loop drains without a full synchronisation)
    std::vector<EventPair> later;
    for (auto& ev : ctx->pending) {
        if (hipEventQuery(ev.b) == hipErrorNotReady) {
            later.push_back(ev);
            continue;
        }
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) ctx->t_ms[ev.slot] += (double)ms;
        ctx->free_events.push_back(ev.a), ctx->free_events.push_back(ev.b);
    }
    (void)hipGetLastError();  // hipErrorNotReady is recorded as the thread's last error
    ctx->pending.swap(later);
    // the stamped batches (run_residuals): ticks of the device's wall clock, copied once by the call that just synchronised
    if (ctx->batch_ticks_in_flight && hipStreamQuery(ctx->stream) == hipSuccess) {
        const unsigned long long now = ctx->rb()->batch_ticks;
        if (ctx->wall_clock_khz > 0) ctx->t_ms[T_RESIDUAL] += (double)(now - ctx->batch_ticks_seen) / (double)ctx->wall_clock_khz;
        ctx->batch_ticks_seen = now, ctx->batch_ticks_in_flight = false;
    }
    (void)hipGetLastError();
}
hipError_t enqueue_batch_ticks(dmsa_ctx* ctx) {
    if (!ctx->batch_ticks_dirty) return hipSuccess;
    ctx->batch_ticks_dirty = false, ctx->batch_ticks_in_flight = true;
    return hipMemcpyAsync(&ctx->rb()->batch_ticks, ctx->d_batch_clock.p, 8, hipMemcpyDeviceToHost, ctx->stream);
}

// Host synchronisation on the critical path of an iteration: polling the stream avoids the ~20-30 us wake-up latency of a
// blocking hipStreamSynchronize (there are four such points per iteration).
hipError_t sync_spin(hipStream_t stream) {
    hipError_t e;
    while ((e = hipStreamQuery(stream)) == hipErrorNotReady) {
    }
    (void)hipGetLastError();  // hipErrorNotReady is recorded as the thread's last error: do not leave it for other HIP users (torch)
    return e;
}

int set_device(dmsa_ctx* ctx) {
    HIPCHK(hipSetDevice(ctx->device));
    return DMSA_OK;
}

int num_params(const dmsa_ctx* ctx) { return ctx->model == MODEL_WINDOW ? ctx->win.ctrl.num_params() : ctx->key.frames.num_params(); }
PoseChain& chain(dmsa_ctx* ctx) { return ctx->model == MODEL_WINDOW ? ctx->win.ctrl : ctx->key.frames; }
int num_extra_rows(const dmsa_ctx* ctx) { return ctx->model == MODEL_WINDOW ? ctx->win.num_extra_rows() : ctx->key.num_extra_rows(); }

// numPointsPerSet.cast<float>().array().pow(-1) (Gaussians.h:172) is libm's powf(n, -1.0f) per coefficient (Eigen 3.4.0's scalar_pow_op
// has no packet path), and powf is not correctly rounded: for some n it is one ulp away from 1.0f / n.  The device divides and applies
// what THIS machine's libm says differs, two bits per member count n: 0 same bits, 1 one ulp above, 2 one ulp below, 3 further away
// (never seen; such a count takes the division and the context reports it).  The table is computed once per process and extended on
// demand; a context uploads the range its point count allows.
namespace {
std::mutex g_pow_mutex;
std::vector<uint32_t> g_pow_codes;  // 16 counts per word
int64_t g_pow_n = 0;                // counts covered
int64_t g_pow_far = 0;              // counts whose powf is more than one ulp from the division
}  // namespace
int upload_powm1_codes(dmsa_ctx* ctx, int64_t counts) {
    counts = (counts + 15) / 16 * 16;
    if (counts <= ctx->pow_n) return DMSA_OK;
    std::vector<uint32_t> words;
    {
        std::lock_guard<std::mutex> lock(g_pow_mutex);
        if (counts > g_pow_n) {
            const int64_t from = g_pow_n;
            g_pow_codes.resize((size_t)(counts / 16), 0u);
            std::atomic<int64_t> far{0};
            workers(ctx).run_all([&](int t, int nt) {
                const int64_t w0 = from / 16 + (counts / 16 - from / 16) * t / nt, w1 = from / 16 + (counts / 16 - from / 16) * (t + 1) / nt;
                volatile float minus_one = -1.0f;  // (volatile: no folding of the call into a division)
                for (int64_t w = w0; w < w1; ++w) {
                    uint32_t word = 0;
                    for (int k = 0; k < 16; ++k) {
                        const int64_t nn = 16 * w + k;
                        if (nn == 0) continue;
                        const float x = (float)nn, a = powf(x, minus_one), d = 1.0f / x;
                        int32_t ia, id;
                        std::memcpy(&ia, &a, 4), std::memcpy(&id, &d, 4);
                        const uint32_t code = ia == id ? 0u : (ia == id + 1 ? 1u : (ia == id - 1 ? 2u : 3u));
                        if (code == 3u) far += 1;
                        word |= code << (2 * k);
                    }
                    g_pow_codes[(size_t)w] = word;
                }
            });
            g_pow_n = counts, g_pow_far += far.load();
        }
        words.assign(g_pow_codes.begin(), g_pow_codes.begin() + counts / 16);
        if (g_pow_far > 0) ctx->err = "warning: this libm's powf(n, -1) is more than one ulp away from 1 / n for some n; those counts use the division";
    }
    HIPCHK(ctx->d_pow_codes.ensure(words.size() * 4));
    HIPCHK(hipMemcpy(ctx->d_pow_codes.p, words.data(), words.size() * 4, hipMemcpyHostToDevice));
    ctx->pow_n = counts;
    return DMSA_OK;
}
// allocate everything whose size depends only on the point count
int alloc_point_buffers(dmsa_ctx* ctx, int64_t n_points) {
    const size_t n = (size_t)n_points;
    HIPCHK(ctx->d_global.ensure(n * 16, ctx->model != MODEL_NONE /* a reservation: the resident problem's global points stay readable */));
    const size_t nb = (n + kAabbBlock - 1) / kAabbBlock;
    HIPCHK(ctx->d_aabb.ensure(nb * 8 * sizeof(float)));
    // lattice tables and counts in one block, in the layout of the host's Readback: sync A reads it back in one copy (debug switch one_readback)
    if (!ctx->d_readback.p) {
        HIPCHK(ctx->d_readback.ensure(dmsa_ctx::kReadbackBytes));
        HIPCHK(hipMemset(ctx->d_readback.p, 0, ctx->d_readback.cap));
        ctx->d_lattice.p = ctx->d_readback.as<char>() + offsetof(dmsa_ctx::Readback, lattice);
        ctx->d_counts.p = ctx->d_readback.as<char>() + offsetof(dmsa_ctx::Readback, g);  // GaussCounts | SerialCounts merged, level 0, level 1
    }
    HIPCHK(ctx->d_keying.ensure(2 * sizeof(LatticeTable)));  // (keys_ahead: filled behind the first voxelisation)
    // the codes and indices of both levels live in ONE array of 2n entries (level 1 behind level 0): they are sorted together
    HIPCHK(ctx->d_code[0].ensure(2 * n * 8));
    HIPCHK(ctx->d_idx[0].ensure(2 * n * 4));
    HIPCHK(ctx->d_code_s[0].ensure(2 * n * 8));
    HIPCHK(ctx->d_idx_s[0].ensure(2 * n * 4));
    for (int l = 0; l < 2; ++l) {
        HIPCHK(ctx->d_leaf_incl[l].ensure(n * 4));
        HIPCHK(ctx->d_leaf_start[l].ensure((n + 1) * 4));
        HIPCHK(ctx->d_head[l].ensure(n * 4));
        HIPCHK(ctx->d_slot_acc[l].ensure(2 * n * 4));
        HIPCHK(ctx->d_slot_cnt[l].ensure(2 * n * 4));
        HIPCHK(ctx->d_gauss_of_slot[l].ensure(2 * n * 4));
        HIPCHK(ctx->d_memb_of_slot[l].ensure(2 * n * 4));
        HIPCHK(ctx->d_sort_tmp[l].ensure(sort_pairs_temp_bytes(2 * n)));
        HIPCHK(ctx->d_scan_tmp[l].ensure(scan_temp_bytes(2 * n)));
    }
    // memberships: every point belongs to at most one set per resolution
    HIPCHK(ctx->d_memb_local.ensure(2 * n * 16));
    HIPCHK(ctx->d_memb_idx.ensure(2 * n * 4));
    HIPCHK(ctx->d_memb_g.ensure(2 * n * 4));
    HIPCHK(ctx->d_seg_off.ensure((2 * n + 2) * 4));
    // sets have >= 2 members (two distinct ids) -- except the second half of a splitSet, which may keep a single member when
    // min_num_points_per_set <= 1: size for one set per membership
    HIPCHK(ctx->d_info12.ensure((2 * n + 16) * 48));
    // one entry per Gaussian, and M can approach 2n (see d_info12 above)
    HIPCHK(ctx->d_order.ensure((2 * n + 16) * 4));
    HIPCHK(ctx->d_order_level.ensure((2 * n + 16) * 4));
    for (int l = 0; l < 2; ++l) HIPCHK(ctx->d_gauss_size[l].ensure((n + 8) * 4));
    HIPCHK(ctx->d_fit_sums.ensure((2 * n + 16) * 6 * 4));
    CHK(upload_powm1_codes(ctx, (int64_t)n + 1));
    HIPCHK(ctx->d_memb_q.ensure(3 * (2 * n + 16) * 4));
    HIPCHK(ctx->d_gauss_rows.ensure((2 * n + 16) * 8));
    return DMSA_OK;
}

// The constants of the problem model the device-resident loop reads (IMU factors / gravity and odometry measurements) and the kernel
// argument that points at them.  Called by upload_commit for the host model (ctx->win / ctx->key) that upload_begin initialised.
int upload_loop_model(dmsa_ctx* ctx, Model model) {
    auto put = [&](DevBuf& buf, const void* src, size_t bytes) -> int {
        HIPCHK(buf.ensure(bytes + 16));
        if (bytes) HIPCHK(hipMemcpy(buf.p, src, bytes, hipMemcpyHostToDevice));
        return DMSA_OK;
    };
    LoopModel m{};
    if (model == MODEL_WINDOW) {
        const WindowHost& w = ctx->win;
        m.model = 1, m.n = w.ctrl.n, m.P = w.ctrl.num_params(), m.extra = w.num_extra_rows();
        m.stamps = ctx->d_stamps.as<double>(), m.fhw = ctx->d_fhw.as<double>(), m.traj_time = ctx->d_trajtime.as<double>();
        m.imu = w.imu_consts();
        m.imu.param_indices = nullptr, m.imu.preint_rot = m.imu.preint_pos = m.imu.preint_vel = m.imu.cov_inv = nullptr;
        if (w.use_imu) {
            CHK(put(ctx->d_imu_idx, w.param_indices.data(), w.param_indices.size() * 4));
            CHK(put(ctx->d_imu_rot, w.preint_rot.data(), w.preint_rot.size() * 8));
            CHK(put(ctx->d_imu_pos, w.preint_pos.data(), w.preint_pos.size() * 8));
            CHK(put(ctx->d_imu_vel, w.preint_vel.data(), w.preint_vel.size() * 8));
            CHK(put(ctx->d_imu_cov, w.cov_inv.data(), w.cov_inv.size() * 8));
            m.imu.param_indices = ctx->d_imu_idx.as<int>(), m.imu.preint_rot = ctx->d_imu_rot.as<double>(), m.imu.preint_pos = ctx->d_imu_pos.as<double>();
            m.imu.preint_vel = ctx->d_imu_vel.as<double>(), m.imu.cov_inv = ctx->d_imu_cov.as<double>();
        }
    } else {
        const KeyframeHost& k = ctx->key;
        m.model = 2, m.n = k.frames.n, m.P = k.frames.num_params(), m.extra = k.num_extra_rows();
        m.key = k.row_consts();
        m.key.measured_gravity = nullptr, m.key.gravity_plausible = nullptr, m.key.odom_transl = nullptr, m.key.odom_orient_mat = nullptr;
        if (k.use_gravity) {
            CHK(put(ctx->d_key_grav, k.measured_gravity.data(), k.measured_gravity.size() * 8));
            CHK(put(ctx->d_key_plaus, k.gravity_plausible.data(), k.gravity_plausible.size() * 4));
            m.key.measured_gravity = ctx->d_key_grav.as<double>(), m.key.gravity_plausible = ctx->d_key_plaus.as<int>();
        }
        if (k.use_odometry) {
            CHK(put(ctx->d_key_odom_t, k.odom_transl.data(), k.odom_transl.size() * 8));
            CHK(put(ctx->d_key_odom_R, k.odom_orient_mat.data(), k.odom_orient_mat.size() * 8));
            m.key.odom_transl = ctx->d_key_odom_t.as<double>(), m.key.odom_orient_mat = ctx->d_key_odom_R.as<double>();
        }
    }
    ctx->loop_model = m;
    return DMSA_OK;
}

// ---- StreamDep (dmsa_ctx.h) ----
StreamDep::~StreamDep() {
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
}
hipError_t StreamDep::create_events() {
    for (int e = 0; e < num_events; ++e)
        if (hipError_t rc = hipEventCreateWithFlags(&ev[e], hipEventDisableTiming); rc != hipSuccess) return rc;
    return hipSuccess;
}
bool StreamDep::by_counter() const { return ctx->dbg.device_sync != 0; }
uint32_t* StreamDep::counter() const { return ctx->d_sync.as<uint32_t>() + slot; }
int32_t* StreamDep::timed_out(const dmsa_ctx* ctx) { return ctx->d_sync.as<int32_t>() + SYNC_TIMED_OUT; }
uint32_t* StreamDep::kernel_signal(hipStream_t from, hipStream_t to, int signals) {
    if (from == to || !by_counter()) return nullptr;
    expected += (uint32_t)signals;
    return counter();
}
int StreamDep::signal(hipStream_t from, hipStream_t to, int e) {
    if (from == to) return DMSA_OK;
    if (by_counter())
        launch_sync_signal(counter(), from), expected += 1;
    else
        HIPCHK(hipEventRecord(ev[e], from));
    return DMSA_OK;
}
int StreamDep::wait(hipStream_t to, hipStream_t from, int e, const WaitCarry* carry) { return from == to ? DMSA_OK : wait_on(to, e, carry); }
int StreamDep::wait_on(hipStream_t to, int e, const WaitCarry* carry) {
    if (!by_counter()) {
        HIPCHK(hipStreamWaitEvent(to, ev[e], 0));
        return DMSA_OK;
    }
    assert(expected != 0 && "dev_sync.h rule (1): no signal was enqueued for this wait");
    ctx->wait_seq += 1;
    uint32_t target = expected;
    int spins = 1 << 23;
    if (ctx->dbg.sync_fault > 0 && ctx->wait_seq == ctx->dbg.sync_fault) target += 1, spins = 1 << 12;  // test hook: a signal that never comes
    launch_sync_wait(counter(), target, timed_out(ctx), to, spins, carry ? carry->second_wait.wait_counter : nullptr, carry ? carry->second_wait.wait_target : 0,
                     carry ? carry->pass_on : nullptr, carry ? carry->stamp : BatchStamp());
    return DMSA_OK;
}
void StreamDep::kernel_wait(DevSync& sy) {
    assert(expected != 0 && "dev_sync.h rule (1): no signal was enqueued for this wait");
    sy.wait_counter = counter(), sy.wait_target = expected, sy.timed_out = timed_out(ctx);
}
void StreamDep::inside_kernel(uint32_t** c, uint32_t* target, int32_t** flag) { *c = counter(), *target = ++expected, *flag = timed_out(ctx); }
int StreamDep::signal_owed(hipStream_t from, hipStream_t to) {
    owed = from != to;
    return signal(from, to);
}
int StreamDep::wait_owed(hipStream_t to) {
    if (!owed) return DMSA_OK;
    owed = false;
    return wait_on(to, 0);
}
void StreamDep::kernel_wait_owed(DevSync& sy) {
    if (owed && by_counter()) kernel_wait(sy), owed = false;
}
bool sync_wait_timed_out(dmsa_ctx* ctx, std::string* what) {
    if (!ctx->d_sync.p) return false;
    int32_t t[3] = {0, 0, 0};
    const bool read = hipDeviceSynchronize() == hipSuccess && hipMemcpy(t, StreamDep::timed_out(ctx), sizeof(t), hipMemcpyDeviceToHost) == hipSuccess;
    if (read && t[0] == 0) return false;
    if (what) *what = read ? "waited for " + std::to_string(t[1]) + ", counter at " + std::to_string(t[2]) : std::string("flag unreadable");
    // start over: nothing is in flight after the synchronisation above
    (void)hipMemset(ctx->d_sync.p, 0, SYNC_SLOTS * 4);
    (void)hipDeviceSynchronize();
    for (StreamDep* d : ctx->deps) d->reset();
    return true;
}
void write_back_poses(const PoseChain& c, double* rel_o, double* rel_t) {
    std::copy(c.rel_o.begin(), c.rel_o.end(), rel_o);
    std::copy(c.rel_t.begin(), c.rel_t.end(), rel_t);
}

// The debug switches (include/dmsa_debug.h documents them): one row per field of dmsa_debug_options, in struct order.  Defaults, DMSA_DEBUG names
// and accepted ranges all come from this table; a value outside [lo, hi] is moved to the nearer end.
namespace {
constexpr int32_t kMin = std::numeric_limits<int32_t>::min(), kMax = std::numeric_limits<int32_t>::max();  // no limit
struct Switch {
    const char* name;
    size_t offset;
    int32_t def, lo, hi;
    bool low_is_default;  // a value below lo becomes the default instead of lo
};
#define SW(field, ...) {#field, offsetof(dmsa_debug_options, field), __VA_ARGS__}
constexpr Switch kSwitches[] = {
    SW(device_loop, 1, kMin, kMax),
    SW(dual_stream, 1, kMin, kMax),
    SW(serial_streams, 3, 1, 3),
    SW(merge_sort, 0, -1, 1),  // by size / two sorts / one sort: any negative value means -1, any positive one 1
    SW(key_compress, 1, kMin, kMax),
    SW(fused_segments, 1, kMin, kMax),
    SW(sort_prehist, 0, kMin, kMax),
    SW(overlap_batch, 1, kMin, kMax),
    SW(serial_tree, 1, 0, 3),
    SW(host_threads, 16, 1, 64),
    SW(solve_threads, 12, 1, 16),
    SW(host_timeline, 0, kMin, kMax),
    SW(trace_time, 0, kMin, kMax),
    SW(fused_leaf_scan, 1, kMin, kMax),
    SW(device_sync, 1, kMin, kMax),
    SW(shared_rotations, 1, kMin, kMax),
    SW(eval_skip, 1, kMin, kMax),
    SW(sync_fault, 0, kMin, kMax),
    SW(speculation_fault, 0, kMin, kMax),
    SW(voxel_coherence, 0, kMin, kMax),
    SW(lm_stream, 1, kMin, kMax),
    SW(stream_priority, 0, kMin, kMax),
    SW(gap_stamps, 0, kMin, kMax),
    SW(lattice_hint, 1, kMin, kMax),
    SW(fit_classes, 7, kMin, kMax),
    SW(eigen_l1_bytes, 32 * 1024, 4096, kMax, true),  // (the default is Eigen's own when cpuid reports nothing)
    SW(small_threshold, 0, kMin, kMax),
    SW(skip_stats, 0, kMin, kMax),
    SW(small_voxel, 0, kMin, kMax),
    SW(long_split, 1, kMin, kMax),
    SW(long_log2, 0, kMin, kMax),
    SW(sort_items, 0, kMin, kMax),
    SW(trial_rows_aside, 1, kMin, kMax),
    // ---- behind the public struct: switches of dmsa_switches (dmsa_ctx.h) that have no field there, set through DMSA_DEBUG by name only ----
    {"batch_stamps", sizeof(dmsa_debug_options), 1, 0, 1},      // (measured: profiles/r15_batch_stamps_ab.txt)
    {"one_readback", sizeof(dmsa_debug_options) + 4, 1, 0, 1},  // (the same file)
    {"fit_by_level", sizeof(dmsa_debug_options) + 8, 1, 0, 2},  // (measured: profiles/r11_fit_by_level_ab.txt)
    {"next_head", sizeof(dmsa_debug_options) + 12, 1, 0, 3},    // (measured: profiles/r18_next_head_ab.txt)
    {"ne_triangle", sizeof(dmsa_debug_options) + 16, 1, 0, 1},  // (measured: profiles/r20_ne_triangle_ab.txt)
    {"keys_ahead", sizeof(dmsa_debug_options) + 20, 1, 0, 2},   // (measured: profiles/r24_keys_ahead_ab.txt)
};
#undef SW
constexpr size_t kNumSwitches = sizeof(kSwitches) / sizeof(kSwitches[0]);
static_assert(kNumSwitches == sizeof(dmsa_switches) / 4 && sizeof(dmsa_switches) == sizeof(dmsa_debug_options) + 24, "one table row per field of dmsa_switches");
constexpr bool switches_in_struct_order() {
    for (size_t i = 0; i < kNumSwitches; ++i)
        if (kSwitches[i].offset != 4 * i) return false;
    return true;
}
static_assert(switches_in_struct_order(), "row i of the table describes field i of dmsa_switches");
// every row, of a context's switches; the rows of the public struct alone, of a caller's struct
int32_t& value(dmsa_switches* o, const Switch& sw) { return *reinterpret_cast<int32_t*>(reinterpret_cast<char*>(o) + sw.offset); }
bool is_public(const Switch& sw) { return sw.offset < sizeof(dmsa_debug_options); }
int32_t& public_value(dmsa_debug_options* o, const Switch& sw) { return *reinterpret_cast<int32_t*>(reinterpret_cast<char*>(o) + sw.offset); }
}  // namespace

extern "C" {

void dmsa_default_debug_options(dmsa_debug_options* o) {
    if (!o) return;
    for (const Switch& sw : kSwitches)
        if (is_public(sw)) public_value(o, sw) = sw.def;
}
// DMSA_DEBUG="name=value,name=value": the one environment variable of the library (include/dmsa_debug.h)
static void apply_named_switches(dmsa_switches* o, const char* e, const char* where) {
    if (!e) return;
    std::string text(e);
    size_t at = 0;
    while (at < text.size()) {
        size_t end = text.find(',', at);
        if (end == std::string::npos) end = text.size();
        const std::string item = text.substr(at, end - at);
        const size_t eq = item.find('=');
        if (eq != std::string::npos) {
            const std::string name = item.substr(0, eq);
            bool known = false;
            for (const Switch& sw : kSwitches)
                if (name == sw.name) value(o, sw) = std::atoi(item.c_str() + eq + 1), known = true;
            if (!known) std::fprintf(stderr, "[dmsa] %s: unknown switch '%s' ignored\n", where, name.c_str());
        }
        at = end + 1;
    }
}
int dmsa_create(int device, uint32_t flags, dmsa_ctx** out) { return dmsa_create_ex(device, flags, nullptr, out); }
// dmsa_create_ex predates the size argument: its callers may hold the round-5 struct, which ends where small_voxel begins.  Only that
// prefix is read; the fields appended since keep their defaults (a caller that sets them uses dmsa_create_ex2 with sizeof).
int dmsa_create_ex(int device, uint32_t flags, const dmsa_debug_options* options, dmsa_ctx** out) {
    return dmsa_create_ex2(device, flags, options, (uint32_t)offsetof(dmsa_debug_options, small_voxel), out);
}
int dmsa_create_ex2(int device, uint32_t flags, const dmsa_debug_options* options, uint32_t options_bytes, dmsa_ctx** out) {
    return dmsa_create_named(device, flags, options, options_bytes, nullptr, out);
}
// ... and with switches by name ("name=value,name=value", may be NULL), applied on top of the struct: the way to the switches that have no field in it
int dmsa_create_named(int device, uint32_t flags, const dmsa_debug_options* options, uint32_t options_bytes, const char* named, dmsa_ctx** out) {
    if (!out) return DMSA_ERR_INVALID;
    dmsa_switches dbg;
    for (const Switch& sw : kSwitches) value(&dbg, sw) = sw.def;
    if (options) {
        // the struct is append-only since round 6: an older caller's shorter struct sets its leading fields, the rest keeps the defaults
        if (options_bytes < 4 || options_bytes % 4 != 0 || options_bytes > sizeof(dmsa_debug_options)) return DMSA_ERR_INVALID;
        std::memcpy(static_cast<dmsa_debug_options*>(&dbg), options, options_bytes);
    }
    apply_named_switches(&dbg, named, "dmsa_create_named");
    apply_named_switches(&dbg, std::getenv("DMSA_DEBUG"), "DMSA_DEBUG");
    for (const Switch& sw : kSwitches) {
        int32_t& v = value(&dbg, sw);
        v = v < sw.lo ? (sw.low_is_default ? sw.def : sw.lo) : std::min(v, sw.hi);
    }
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return DMSA_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return DMSA_ERR_NO_DEVICE;
    dmsa_ctx* ctx = new (std::nothrow) dmsa_ctx();
    if (!ctx) return DMSA_ERR_NOMEM;
    if (flags & ~(DMSA_FLAG_POSE_TABLE_HOST | DMSA_FLAG_FIXED_ITERS | DMSA_FLAG_MIRROR_SUMS | DMSA_FLAG_STAGE_TIMERS)) {
        delete ctx;
        return DMSA_ERR_INVALID;  // e.g. 0x10, the opt-in fast sums of rounds 1-4: retired, the library has ONE summation order (the reference's)
    }
    ctx->device = device, ctx->flags = flags;
    ctx->dbg = dbg;
    // stream_priority: bit 0 / 1 / 2 = main / second / third stream at the device's highest priority (the wave dispatcher then serves that
    // queue first when kernels of several streams compete for the CUs)
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    auto make_stream = [&](hipStream_t* st, int bit) {
        return hipStreamCreateWithPriority(st, hipStreamNonBlocking, ((dbg.stream_priority >> bit) & 1) ? prio_greatest : prio_least / 2 + prio_greatest / 2);
    };
    bool made = make_stream(&ctx->stream, 0) == hipSuccess && make_stream(&ctx->stream2, 1) == hipSuccess && make_stream(&ctx->stream3, 2) == hipSuccess &&
                hipEventCreateWithFlags(&ctx->ev_counts, hipEventDisableTiming) == hipSuccess;
    for (StreamDep* d : ctx->deps) made = made && d->create_events() == hipSuccess;
    if (!made) {
        dmsa_destroy(ctx);
        return DMSA_ERR_HIP;
    }
    if (ctx->h_rb.ensure(sizeof(dmsa_ctx::Readback), nullptr) != hipSuccess) {
        dmsa_destroy(ctx);
        return DMSA_ERR_NOMEM;
    }
    std::memset(ctx->h_rb.p, 0, sizeof(dmsa_ctx::Readback));
    ctx->h_lattice = ctx->rb()->lattice;
    // counters of the device-side stream dependencies (loop_kernels.h): zero BEFORE any stream of this context can look at them -- the
    // three streams are not ordered among themselves, and a recycled allocation still holds the counts of the context that freed it
    // ... and the tick accumulator of the batch stamps, with the rate of the clock that writes them (kHz: ticks / rate = ms)
    if (hipDeviceGetAttribute(&ctx->wall_clock_khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || ctx->wall_clock_khz <= 0)
        ctx->wall_clock_khz = 0, ctx->dbg.batch_stamps = 0;  // no rate, no stamps: the event pair
    if (ctx->d_sync.ensure(SYNC_SLOTS * 4) != hipSuccess || hipMemsetAsync(ctx->d_sync.p, 0, SYNC_SLOTS * 4, ctx->stream) != hipSuccess ||
        ctx->d_batch_clock.ensure(16) != hipSuccess || hipMemsetAsync(ctx->d_batch_clock.p, 0, 16, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        dmsa_destroy(ctx);
        return DMSA_ERR_HIP;
    }
    *out = ctx;
    return DMSA_OK;
}

void dmsa_destroy(dmsa_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (hipStream_t st : {ctx->stream, ctx->stream2, ctx->stream3})
        if (st) (void)hipStreamSynchronize(st);  // every stream idle before anything is freed
    drain_timers(ctx);
    // what does not release itself: the timers' events, streams, the lazily created parts (DevBuf, PinnedBuf and StreamDep members: delete ctx)
    for (hipEvent_t e : ctx->free_events) (void)hipEventDestroy(e);
    if (ctx->ev_counts) (void)hipEventDestroy(ctx->ev_counts);
    delete ctx->pool;
    pcd_release(ctx);
    delete ctx->sp;
    for (hipStream_t st : {ctx->stream3, ctx->stream2, ctx->stream})
        if (st) (void)hipStreamDestroy(st);
    delete ctx;
}

const char* dmsa_last_error(const dmsa_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

void dmsa_default_settings(dmsa_settings* s) {
    if (!s) return;
    s->num_iter = 15, s->epsilon = 1e-5, s->use_analytic_jacobi = 0, s->step_length_optim = 0.05, s->max_step = 0.01, s->gauss_split = 0;
    s->grid_size_1_factor = 2.0f, s->grid_size_2_factor = 5.0f, s->min_num_points_per_set = 6, s->min_num_gaussians = 30;
    s->lambda_diag = 0.00001f, s->use_centralization = 1;
}

int dmsa_window_upload(dmsa_ctx* ctx, const dmsa_window_problem* p) {
    if (!ctx || !p || p->num_points < 0 || p->num_static < 0) return DMSA_ERR_INVALID;
    if ((p->num_points > 0 && (!p->xyz_local || !p->tform_idx || !p->ring_id)) || (p->num_static > 0 && (!p->xyz_static || !p->ring_id_static))) {
        ctx->err = "invalid window problem (null point arrays)";
        return DMSA_ERR_INVALID;
    }
    return upload_window(ctx, p, WindowPoints::flat(p), StaticPoints::flat(p));
}

int dmsa_keyframes_upload(dmsa_ctx* ctx, const dmsa_keyframe_problem* p) {
    if (!ctx || !p || p->num_frames < 2) return DMSA_ERR_INVALID;
    if (!p->frame_offset || !p->xyz_local || !p->normal_local || !p->ring_id) {
        ctx->err = "invalid keyframe problem (null point arrays)";
        return DMSA_ERR_INVALID;
    }
    if (p->frame_offset[0] != 0) {
        ctx->err = "invalid keyframe problem (frame_offset[0] != 0)";
        return DMSA_ERR_INVALID;
    }
    for (int k = 0; k < p->num_frames; ++k)
        if (p->frame_offset[k + 1] < p->frame_offset[k]) {
            ctx->err = "invalid keyframe problem (frame_offset not non-decreasing)";
            return DMSA_ERR_INVALID;
        }
    return upload_keyframes(ctx, p, p->frame_offset[p->num_frames], nullptr);
}

}  // extern "C"
