// dmsa_ctx.h — the context of libdmsa_hip.so and what its translation units share (internal; nothing here is part of the ABI).
//
//   context.cpp           create / destroy, debug switches, device buffers, timers; the argument checks of the two flat upload entries
//   upload_driver.cpp     how a problem becomes resident, for all six upload entries: upload_begin (withdraws the resident problem, host model,
//                         one sizing function), the named sources of the points, upload_commit (sets the model last); the reservations
//   voxelize_driver.cpp   createGaussianSets at both resolutions + fit (DmsaOptimizer.h:78-96): build_gaussians as a plan (VoxelPlan: every mode
//                         of a build, decided once) and named phases -- lattice, keys and sorts, leaves, gathers, size classes and read-back,
//                         speculated fit, verdict behind sync #2 (with the one redo), rest of the fit, hand-over of the tables to the keying set
//   optimize_loop.cpp     optimizeSet (DmsaOptimizer.h:54-150), in this order: pose tables; residual batches (plan_tiers, long_split_for, one
//                         SerialBatch, fork_tiers / join_tiers); analytic Jacobian; what the two loops share (keyframe_chains_aside, the line
//                         search, HostLmSolve, finish_call); the host-driven loop (optimize_host_loop); the device-resident loop as a plan
//                         (LoopPlan: every mode of a call, decided once), its buffers (LoopBuffers) and the named phases of a DeviceLoop -- seed,
//                         head, side_batch, voxelise, jacobian_batch, normal_equations, lm_step, trial_chains, trial_batch_and_decision,
//                         collect, fold_results; optimize()
//   dmsa_api.cpp          the C ABI of include/dmsa_hip.h (stage-level entry points, whole calls)
//   next_rows_api.cpp     the C ABI of the rows around the hot path (static points, preProcess, window setup, wire formats, keyframe clouds)
//   pcd_export.cpp        PointCloud.pcd: the chunked ASCII writer on top of pcd_kernels.hip
//   copy_back.h           CopyBack and copy_back_chunks: the two-slot way from a device buffer to a file (pcd_file.h), for every PCD writer
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cassert>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dmsa_hip.h"
#include "../../include/dmsa_debug.h"
#include "../../include/dmsa_static_points.h"
#include "../../include/dmsa_window_setup.h"
#include "../../include/dmsa_wire_formats.h"
#include "../../include/dmsa_keyframe_cloud.h"
#include "../../include/dmsa_aos.h"
#include "analytic_jacobian.h"
#include "device_prims.h"
#include "radix_sort_dev.h"
#include "dmsa_kernels.h"
#include "host_math.h"
#include "loop_kernels.h"
#include "pcd_kernels.h"
#include "serial_kernels.h"
#include "static_kernels.h"

using namespace dmsa;  // kernels / host math of this library

// a part of a DevBuf that another member owns (d_readback: the lattice tables and the counts)
struct DevView {
    void* p = nullptr;
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }  // every buffer of a context is released with it (dmsa_destroy: delete ctx)
    // At least `bytes`.  keep: what the old block held moves into a new one (an array of a resident problem; the device is idled first).  Empty after a failure.
    hipError_t ensure(size_t bytes, bool keep = false) {
        if (bytes <= cap) return hipSuccess;
        ++reallocations();  // (hipFree waits for the device: a buffer that grows inside the loop costs an iteration its overlap)
        DevBuf old;
        old.swap(*this);
        if (!keep) old.release();
        const size_t want = bytes + bytes / 8 + 256;
        hipError_t e = old.p ? hipDeviceSynchronize() : hipSuccess;
        if (e == hipSuccess) e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        else p = nullptr;
        if (e == hipSuccess && old.p) e = hipMemcpy(p, old.p, old.cap, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) release();
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
    }
    void swap(DevBuf& o) { std::swap(p, o.p), std::swap(cap, o.cap); }  // a fresh buffer filled, then swapped in: the old block leaves with `o`
    static long long& reallocations() {  // process-wide count of growing ensure() calls (debug switch trace_time prints it per iteration)
        static long long n = 0;
        return n;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// The next epoch of a scratch whose words carry the epoch of the launch that wrote them: never 0, the value of a cleared word.
inline uint32_t next_epoch(uint32_t& e) {
    if (++e == 0) e = 1;
    return e;
}

// The persistent state of one single-pass chained scan (chained_scan.h): a ticket counter and the tiles' entries, cleared only when the
// buffer is new.  Entries carry the epoch of the call that wrote them (0: a cleared word), so a call ignores what earlier calls left
// behind, and the ticket counter runs on.  (After 2^32 calls an epoch comes round again; a word that old would have to survive them.)
struct ChainedScanState {
    DevBuf buf;
    uint32_t epoch = 0, ticket = 0;
    // the next call, of `tiles` tiles with `words` 64-bit words each, enqueued on `s`
    hipError_t begin(size_t tiles, size_t words, hipStream_t s, ChainedScanCall* call) {
        if (const size_t need = 8 * (1 + words * tiles); need > buf.cap) {
            hipError_t e = buf.ensure(need);
            if (e == hipSuccess) e = hipMemsetAsync(buf.p, 0, buf.cap, s);
            if (e != hipSuccess) return e;
            epoch = 0, ticket = 0;
        }
        *call = {buf.as<unsigned long long>(), next_epoch(epoch), ticket};
        ticket += (uint32_t)tiles;
        return hipSuccess;
    }
};

// Pinned host memory, owned like DevBuf owns device memory (released with its owner; the owner makes its device current first).
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { release(); }
    // At least `bytes`; a block that has to grow is allocated with `alloc` bytes (the caller's slack; 0: `bytes`).  `drain` is the stream whose
    // copies may still read the old block, idled before it is freed (null: every earlier use ended with a host wait).  Empty after a failure.
    hipError_t ensure(size_t bytes, hipStream_t drain, size_t alloc = 0) {
        if (bytes <= cap) return hipSuccess;
        hipError_t e = drain ? hipStreamSynchronize(drain) : hipSuccess;
        release();
        if (e != hipSuccess) return e;
        const size_t want = std::max(alloc, bytes);
        e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        else p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr, cap = 0;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};
// The pinned staging area of a context: what an upload packs or gathers for its copies to the device, a pushed scan, the pieces that
// dmsa_get_global_points_aos brings down.  THE REUSE RULE: acquire() before the host writes into the area or a copy into it is enqueued,
// release(stream) behind the last copy enqueued from or into it, on every exit path that enqueued one.  acquire() waits on the host until
// everything in front of the last release() has passed, so no user of the area synchronises a stream for the area's sake, and none has to
// know whether the user before it ended with a host wait.  A user that ends with a host wait of its own takes wait() for it.
class StageArea {
public:
    // at least `bytes`, free to be written; a block that has to grow gets an eighth of slack
    hipError_t acquire(size_t bytes, char** area = nullptr) {
        if (hipError_t e = wait(); e != hipSuccess) return e;
        if (hipError_t e = buf.ensure(bytes, nullptr /* by the rule nothing reads or writes the old block any more */, bytes + bytes / 8); e != hipSuccess) return e;
        if (area) *area = buf.as<char>();
        return hipSuccess;
    }
    // (one stream at a time: every user passes the context's main stream; a second stream would need the first one's wait kept as well)
    void release(hipStream_t stream) {
        assert(!busy_on || busy_on == stream);
        busy_on = stream;
    }
    hipError_t wait() {
        if (!busy_on) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(busy_on);
        if (e == hipSuccess) busy_on = nullptr;
        return e;
    }

private:
    PinnedBuf buf;
    hipStream_t busy_on = nullptr;  // the stream of the last release() that no wait() has passed yet
};
// Four slots of doubles handed out round robin: the staging of small host-to-device copies that nobody waits for (control poses, additional
// rows).  At least one stream synchronisation separates reuse of a slot (4 syncs per iteration).
struct PinnedRing {
    static constexpr size_t kSlots = 4;
    PinnedBuf buf;
    size_t at = 0;
    hipError_t next(size_t count, hipStream_t drain, double** out) {
        if (count > buf.cap / (kSlots * sizeof(double))) {
            hipError_t e = buf.ensure(kSlots * sizeof(double) * (count + count / 2 + 64), drain);
            if (e != hipSuccess) return e;
        }
        *out = buf.as<double>() + at * (buf.cap / (kSlots * sizeof(double)));
        at = (at + 1) % kSlots;
        return hipSuccess;
    }
};

// One dependency between two streams of a context (dev_sync.h), in the mechanism the context uses at the moment: a counter of d_sync where
// dbg.device_sync is set, HIP events otherwise.  The mode is read at every use (optimize() clears device_sync after a wait that timed out and
// runs the call again).  Every operation names the producer's stream `from` and the consumer's stream `to`: where both are one stream
// (dual_stream = 0, serial_streams = 1, a voxel level switched off) stream order holds the dependency and nothing is enqueued in either mode.
// dev_sync.h rule (1), a signal is ENQUEUED before the wait that needs it, is the call sites' to keep: a wait on a slot without a signal asserts.
struct dmsa_ctx;
// what the one wave of a wait kernel may carry besides its own dependency (counters only; with events both stay with their own StreamDep)
struct WaitCarry {
    DevSync second_wait;         // a wait another dependency handed out with kernel_wait / kernel_wait_owed (its wait_* fields; null: none)
    uint32_t* pass_on = nullptr; // a signal another dependency handed out with kernel_signal, given once the wave's waits are through
    BatchStamp stamp;            // the end stamp of a residual batch (dev_sync.h), taken once the wave's waits are through (null: none)
};
class StreamDep {
public:
    StreamDep(dmsa_ctx* c, SyncSlot s, int events) : ctx(c), slot(s), num_events(events) {}
    StreamDep(const StreamDep&) = delete;
    StreamDep& operator=(const StreamDep&) = delete;
    ~StreamDep();
    hipError_t create_events();
    bool by_counter() const;
    // The signal rides on the kernel launched next on `from`, which gives it `signals` times: the counter to hand to that kernel.  Null in event
    // mode (and on one stream): the caller then calls signal() where the events' order wants it.
    uint32_t* kernel_signal(hipStream_t from, hipStream_t to, int signals = 1);
    // behind everything `from` holds now: a one-wave kernel / hipEventRecord(event e)
    int signal(hipStream_t from, hipStream_t to, int e = 0);
    // in front of everything `to` gets from now on: a one-wave kernel for all signals enqueued so far / hipStreamWaitEvent(event e)
    int wait(hipStream_t to, hipStream_t from, int e = 0, const WaitCarry* carry = nullptr);
    // the same wait carried by thread 0 of a kernel of the consumer's stream (counters only; not counted by the debug switch sync_fault)
    void kernel_wait(DevSync& sy);
    // a dependency between the workgroups of ONE kernel: a counter whatever the mode, one signal per launch
    void inside_kernel(uint32_t** counter, uint32_t* target, int32_t** timed_out);
    // A signal whose consumer is not known yet (the pose tables of a batch: whoever reads them first on `to` waits) ...
    int signal_owed(hipStream_t from, hipStream_t to);
    int wait_owed(hipStream_t to);     // ... that reader, on the host's side: nothing if nothing is owed
    void kernel_wait_owed(DevSync& sy);  // ... or inside its kernel: nothing if nothing is owed or in event mode (wait_owed is then still to come)
    void reset() { expected = 0, owed = false; }  // after the counters were zeroed with nothing in flight
    static int32_t* timed_out(const dmsa_ctx* ctx);  // the three words a wait that gives up writes (DevSync::timed_out)

private:
    int wait_on(hipStream_t to, int e, const WaitCarry* carry = nullptr);
    uint32_t* counter() const;
    dmsa_ctx* const ctx;
    const SyncSlot slot;
    const int num_events;  // events of the event mode (0: the dependency exists with counters only)
    hipEvent_t ev[2] = {nullptr, nullptr};
    uint32_t expected = 0;  // signals enqueued so far = the value a wait enqueued now has to see
    bool owed = false;
};

enum Model { MODEL_NONE = 0, MODEL_WINDOW = 1, MODEL_KEYFRAMES = 2 };

enum TimerSlot { T_RESIDUAL = 0, T_VOXEL, T_FIT, T_TABLE, T_NORMAL, T_TOTAL, T_COUNT };

struct EventPair {
    hipEvent_t a, b;
    int slot;
};

// scratch of the static-point functions (include/dmsa_static_points.h); allocated on first use, independent of the resident problem
struct StaticState {
    DevBuf cloud, query, normal, ring, code, idx, code_s, idx_s, pts_sorted, table, flags, sel, scan, sort_tmp, scan_tmp, out_xyz, out_id, offsets, small,
        aabb, lattice, head, incl, leaf_start, counts, rnd, pick;
    // the cell grid currently built over `cloud`
    CellGrid grid{};
    int64_t n_cloud = 0;
    uint32_t num_finite = 0;
    bool key32 = false;
    uint32_t table_mask = 0;
};

// A few persistent host threads for the O(#poses x #evaluations) host math (perturbed pose chains of the keyframe pass, host pose
// tables of the parity path, packing of an upload).  Spawning threads per batch cost ~0.5 ms per iteration; the workers sleep on a
// condition variable between batches.
class WorkerPool {
public:
    explicit WorkerPool(int n) {
        for (int t = 0; t < n; ++t) threads_.emplace_back([this, t]() { run(t); });
    }
    ~WorkerPool() {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& th : threads_) th.join();
    }
    int size() const { return (int)threads_.size(); }
    // fn(worker_index, num_workers) on every worker; returns when all are done
    void run_all(const std::function<void(int, int)>& fn) {
        {
            std::lock_guard<std::mutex> lk(m_);
            fn_ = &fn, pending_ = (int)threads_.size(), ++generation_;
        }
        cv_.notify_all();
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [this]() { return pending_ == 0; });
        fn_ = nullptr;
    }

private:
    void run(int t) {
        long seen = 0;
        while (true) {
            const std::function<void(int, int)>* fn = nullptr;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&]() { return stop_ || generation_ != seen; });
                if (stop_) return;
                seen = generation_, fn = fn_;
            }
            (*fn)(t, (int)threads_.size());
            {
                std::lock_guard<std::mutex> lk(m_);
                if (--pending_ == 0) done_.notify_one();
            }
        }
    }
    std::vector<std::thread> threads_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(int, int)>* fn_ = nullptr;
    int pending_ = 0;
    long generation_ = 0;
    bool stop_ = false;
};

// include/dmsa_window_ring.h: the window's scans resident in HBM (slot s holds up to `cap` points at offset s * cap)
struct WindowRing {
    int num_scans = 0;  // 0: no ring
    int64_t cap = 0;
    int head = 0, filled = 0;  // next slot to overwrite, slots in use
    std::vector<int64_t> count;
    DevBuf xyz, stamp, id;
};

// host-side time stamps of one iteration of optimize() (debug switch host_timeline)
struct HostTimeline {
    bool on = false;  // debug switch host_timeline
    std::vector<std::pair<const char*, std::chrono::steady_clock::time_point>> marks;
    void reset() { marks.clear(); }
    void mark(const char* what) {
        if (on) marks.emplace_back(what, std::chrono::steady_clock::now());
    }
    void print() const {
        if (!on || marks.size() < 2) return;
        std::fprintf(stderr, "[host timeline]");
        for (size_t i = 1; i < marks.size(); ++i)
            std::fprintf(stderr, " %s %.0f |", marks[i].first, std::chrono::duration<double, std::micro>(marks[i].second - marks[i - 1].second).count());
        std::fprintf(stderr, " total %.0f us\n", std::chrono::duration<double, std::micro>(marks.back().second - marks.front().second).count());
    }
};

// The context's switches: the public struct and, behind it, switches without a field there -- DMSA_DEBUG sets them by name, and the public
// struct (an ABI that tests/test_cabi_cpu.py pins field by field) does not grow for an experiment.  One table describes both (context.cpp).
struct dmsa_switches : dmsa_debug_options {
    int32_t batch_stamps = 1;  // a residual batch with a join wait is timed by the device's wall clock, read inside its own kernels (run_residuals); 0: a HIP-event pair around every batch
    int32_t one_readback = 1;  // sync A waits for ONE device-to-host copy of d_readback (voxelize_driver.cpp: readback_copies); 0: counts, lattice tables and IterResult in a copy each
    int32_t fit_by_level = 1;  // each voxel level's size classes, gather and fit behind its own k_leaf_finalize (voxelize_driver.cpp): 1 from 200 000 points on, 2 always; 0: the common order
    int32_t next_head = 1;     // device loop, window without IMU rows: an iteration's base table is adopted from the line search's trial tables instead of computed (optimize_loop.cpp): 1, 2 on; 3 also checks; 0: computed
    int32_t ne_triangle = 1;   // normal equations up to 64 parameters: block sums of the elements i <= j only, from k_normal_eq_source, mirrored by the consumer (dmsa_kernels.hip); 0: k_normal_eq_partial
    int32_t keys_ahead = 1;    // the key kernels and sorts of a speculated voxelisation start behind the transform, on the lattice tables the previous one ended with, beside k_lattice; the host compares the tables at sync #2 (voxelize_driver.cpp): 1, 2 wherever possible; 0: behind k_lattice
};

// What a voxelisation (build_gaussians, voxelize_driver.cpp) leaves behind for the next one of the same context: the guesses its speculations
// start from.  An upload forgets them (forget), a redo withdraws some of them (redo); nothing else resets a field by name.
struct VoxelState {
    int depth_guess[2] = {-1, -1};   // tree depths of the previous voxelisation (speculation: saves one host sync)
    int bits_guess[2] = {-1, -1};    // leaf-code widths of the previous voxelisation
    bool lattice_hint_valid = false;  // d_lattice holds the tables of an earlier voxelisation of this context (k_lattice verifies them before it replays)
    // keys_ahead: the host's side of the keying set (dmsa_ctx::d_keying)
    LatticeTable h_keying[2]{};
    bool keying_valid = false;  // d_keying / h_keying hold the tables of the previous voxelisation, of keying_n points (not behind an upload or a redo)
    int64_t keying_n = 0;
    bool keying_host_valid = false;  // h_keying holds the tables of the previous voxelisation (the device copy is made only when the next build may go ahead)
    int keying_streak = 0;           // consecutive voxelisations whose tables equalled the previous one's (rule of keys_ahead = 1, voxelize_driver.cpp)
    bool fit_guess_valid = false;  // dmsa_ctx::serial_counts of the previous voxelisation may size this one's speculative fit launches
    SerialCounts serial_counts_level[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};  // fit_by_level: the same per level (valid if fit_guess_level)
    bool fit_guess_level = false;

    // a new cloud was uploaded: the sort widths, the keying set and the fit's grids are another cloud's
    void forget() {
        depth_guess[0] = depth_guess[1] = -1;
        keying_valid = false, keying_host_valid = false, keying_streak = 0;
        fit_guess_valid = false, fit_guess_level = false;
    }
    // A speculation of a build did not hold and `rerun` builds again: the width guesses are withdrawn in front of it, so that it waits for the
    // true ones (sync #1), and -- forget_keying -- the keying set it leaves is not used: the next build runs in the common order as well, and
    // the streak starts again.
    template <class Rerun>
    int redo(bool forget_keying, Rerun&& rerun) {
        depth_guess[0] = depth_guess[1] = -1;
        const int rc = rerun();
        if (forget_keying) keying_valid = false, keying_streak = 0;
        return rc;
    }
};

struct dmsa_ctx {
    int device = 0;
    uint32_t flags = 0;
    WindowRing ring;
    dmsa_switches dbg{};  // include/dmsa_debug.h: normalised and fixed at dmsa_create(_ex, _ex2); optimize() alone clears device_sync after a wait that timed out
    hipStream_t stream = nullptr, stream2 = nullptr;  // stream2 carries the second voxel level only
    hipStream_t stream3 = nullptr;                    // the short tier of the correspondence kernels (debug switch serial_streams: 2 = with the throughput tier on stream2, 1 = everything on `stream`)
    // the stream dependencies of an iteration, one per SyncSlot (dev_sync.h says what each orders)
    StreamDep tier_fork{this, SYNC_TIER_FORK, 1}, tier_join{this, SYNC_TIER_JOIN, 2} /* event 0: stream2, 1: stream3 */, loop_state{this, SYNC_LOOP_STATE, 1},
        tables{this, SYNC_TABLES, 1}, classes{this, SYNC_CLASSES, 1}, lattice{this, SYNC_LATTICE, 1}, level1{this, SYNC_LEVEL1, 1}, small_l0{this, SYNC_SMALL_L0, 0},
        trial_step{this, SYNC_TRIAL_STEP, 0}, trial_rows{this, SYNC_TRIAL_ROWS, 0}, sizes0{this, SYNC_SIZES0, 1}, sizes1{this, SYNC_SIZES1, 1},
        classes0{this, SYNC_CLASSES0, 1}, classes1{this, SYNC_CLASSES1, 1}, fit1{this, SYNC_FIT1, 1};
    StreamDep* const deps[15] = {&tier_fork, &tier_join, &loop_state, &tables, &classes, &lattice, &level1, &small_l0, &trial_step, &trial_rows,
                                 &sizes0, &sizes1, &classes0, &classes1, &fit1};
    int tablesT_batch = 0;        // d_tablesT holds the transposed tables of a batch of this size (0: stale)
    hipEvent_t ev_counts = nullptr;  // the counts of a voxelisation have arrived (the host waits for it)
    std::string err;

    Model model = MODEL_NONE;
    int64_t n = 0, N = 0, S = 0;  // total points, moving points, static points
    int rows = 0;                 // pose-table rows incl. the identity row (n_total+1 or F+1)
    WindowHost win;
    KeyframeHost key;
    bool centralized = false;
    float min_grid_size = 0.3f;

    // device-resident problem
    DevBuf d_local, d_nlocal, d_ring, d_global, d_nglobal;
    // pose tables of the current batch
    DevBuf d_tables, d_ctrl, d_stamps, d_fhw, d_trajtime;
    int batch = 0;
    // pinned staging ring for the per-batch control poses (so the H2D copy needs no host synchronisation)
    PinnedRing h_pin, h_xpin;  // (h_xpin: the same for the additional rows of a batch)
    std::vector<float> h_tables;
    StageArea h_stage;  // pinned staging of the uploads and of the strided write-back, with its reuse rule
    // voxelisation
    // per-resolution scratch: the two voxelisations of an iteration run concurrently on `stream` and `stream2`
    DevBuf d_aabb, d_code[2], d_idx[2], d_code_s[2], d_idx_s[2], d_head[2], d_leaf_incl[2], d_leaf_start[2], d_slot_acc[2], d_slot_cnt[2],
        d_gauss_of_slot[2], d_memb_of_slot[2], d_pos_slot_rank[2], d_nsorted[2], d_pair_d[2], d_sort_tmp[2], d_scan_tmp[2];
    // Small device->host read-backs land in PINNED memory: an async copy into pageable memory blocks the host for 20-30 us.
    // Up to `errs` the struct is also the layout of the device block d_readback, which sync A brings over in one copy (debug switch one_readback).
    struct Readback {
        LatticeTable lattice[2];
        GaussCounts g;
        SerialCounts sc;  // d_counts holds the two structs back to back ...
        SerialCounts sc_level[2];  // ... and behind them the size classes of each level on its own (fit_by_level)
        IterResult prev;  // device loop: what k_loop_finish decided last (it writes the slot beside d_results[iter])
        double errs[16];
        unsigned long long batch_ticks;  // the tick accumulator of the batch stamps, as the call's last copy found it
    };
    static constexpr size_t kReadbackBytes = offsetof(Readback, errs);
    DevBuf d_readback;             // LatticeTable[2] | GaussCounts | SerialCounts x 3 | IterResult (hipMalloc aligns it to 256 bytes)
    DevView d_lattice, d_counts;   // views into d_readback (alloc_point_buffers)
    IterResult* d_prev_result() const { return reinterpret_cast<IterResult*>(d_readback.as<char>() + offsetof(Readback, prev)); }
    PinnedBuf h_rb;
    Readback* rb() const { return h_rb.as<Readback>(); }
    PinnedBuf h_Hp;                     // (P+1)^2 read-back of the normal equations
    LatticeTable* h_lattice = nullptr;  // = rb()->lattice
    ChainedScanState seg_state[2];   // look-back state of k_leaf_segments (one word per tile), per level
    ChainedScanState fin_state[2];   // the same for k_leaf_finalize (four words per tile)
    bool key32[2] = {false, false};  // leaf codes are 32-bit (both levels share the width: they are sorted together)
    // level views into the shared code / index arrays (level 1 starts n entries behind level 0)
    void* code_v[2] = {nullptr, nullptr};
    void* code_s_v[2] = {nullptr, nullptr};
    uint32_t* idx_v[2] = {nullptr, nullptr};
    uint32_t* idx_s_v[2] = {nullptr, nullptr};
    double level_res[2] = {0, 0};
    // Gaussians
    DevBuf d_memb_local, d_memb_idx, d_memb_g, d_seg_off, d_info12;
    DevBuf d_sv_stamps;  // debug switch gap_stamps = 3: phase stamps of k_voxel_small
    DevBuf d_long_split;  // scratch of the latency tier's wide second pass (serial_kernels.h: LongSplit)
    size_t long_split_items = 0;
    uint32_t long_split_epoch = 0;
    DevBuf d_order;  // reference-order path: Gaussians by descending size class
    DevBuf d_gauss_size[2];  // fit_by_level: members of every Gaussian of a level, by its index inside the level (k_leaf_finalize)
    DevBuf d_order_level;    // ... and the Gaussians of each level by descending size class: level 0 at [0], level 1 at [n + 8]
    DevBuf d_tablesT;                                          // pose tables of the current batch, transposed ([row][evaluation][12])
    bool order_valid = false;
    DevBuf d_gap_stamps;         // debug switch gap_stamps: 16 wall-clock slots
    VoxelState vox;  // what a voxelisation leaves for the next one of this context
    int64_t lattice_hints_held = 0, lattice_replays = 0;
    // keys_ahead: the KEYING set of lattice tables -- what the previous voxelisation of this context ended with -- in a buffer of its own, so that
    // key kernels and everything downstream of them can read it while k_lattice writes this cloud's tables into d_lattice.  Nothing writes it
    // while such a kernel can run, but the key kernel its code_or; it is refreshed by a copy on the main stream behind a voxelisation in the
    // common order.  vox.h_keying is the host's copy, which the verdict at sync #2 compares the read-back tables with.
    DevBuf d_keying;
    int64_t keys_ahead_held = 0, keys_ahead_redone = 0;  // (voxelisation, level) pairs keyed ahead whose table stood; voxelisations keyed ahead and redone
    DevBuf d_fit_sums;           // six centred product sums per Gaussian (fit kernels -> finish kernel)
    DevBuf d_memb_q;             // fit: global x | y | z of the members of Gaussians too long for the fit's LDS chunk, [3][2n + 16] floats
    DevBuf d_pow_codes;          // two bits per member count n: how libm's powf(n, -1) differs from 1.0f / n (context.cpp: upload_powm1_codes)
    int64_t pow_n = 0;           // counts covered by d_pow_codes
    DevBuf d_gauss_rows;         // (smallest, largest) pose-table row among the members of every Gaussian, identity row excluded (fit kernel)
    DevBuf d_row_range;          // per evaluation of the Jacobian batch: (first, last) pose-table row that can differ from evaluation 0's (loop chain + pose-table kernels)
    DevBuf d_skip_stats;         // per evaluation of the Jacobian batch: pairs (Gaussian, evaluation) not computed, pairs that differed under eval_skip = 2
    int skip_stats_evals = 0;
    DevBuf d_code_prev[2], d_coh_count;  // debug switch voxel_coherence: last voxelisation's leaf codes per level, and a counter of changed codes
    LatticeTable coh_lattice[2]{};
    bool coh_valid[2] = {false, false}, coh_key32[2] = {false, false}, coh_pending[2] = {false, false}, coh_count_zeroed = false;
    int64_t coh_n[2] = {0, 0};
    int64_t coh_compared = 0, coh_lattice_changes = 0;
    DevBuf d_split_stats;        // splitSet search: 64 x 64 pair blocks looked at / skipped by the cone bound (k_split_pairs)
    int64_t skip_pairs = 0;      // pairs the eval_skip logic looked at since the context was created
    SerialCounts serial_counts{0, 0, 0, 0};  // the size classes of the current Gaussians (vox.fit_guess_valid: they may size the next speculated fit)
    bool E_is_jacobian = false;  // the matrix-core normal equations (P > 64) rewrote the residual batch as the columns of [J | e0]
    bool aabb_fresh = false;  // d_aabb / the zeroed counters belong to the current d_global (launch_transform_aabb ran last)
    const float* base_table = nullptr;  // the pose table d_global was computed with (the fit re-derives the members' global coordinates from it)
    // ---- device-resident optimizeSet loop (loop_kernels.h) ----
    LoopModel loop_model{};      // built at upload: device pointers to the model's constants
    DevBuf d_imu_idx, d_imu_rot, d_imu_pos, d_imu_vel, d_imu_cov;           // window model, IMU factor rows
    DevBuf d_key_grav, d_key_plaus, d_key_odom_t, d_key_odom_R;             // keyframe model, gravity / odometry rows
    DevBuf d_loop_state;   // three chain states: start of the iteration, after the Jacobian batch, after the line search
    DevBuf d_loop_vec;     // paramVec[P] | step[P]
    DevBuf d_ctrl0;        // global poses of the base table (n x 6)
    DevBuf d_table0;       // the base pose table (own buffer: the Jacobian batch's tables are written beside the fit that still reads it)
    DevBuf d_trial_tables; // next_head: the nine row-major pose tables of the line search, kept until the next iteration has adopted one (d_tables is the Jacobian batch's by then)
    DevBuf d_head_check, d_head_mismatches;  // next_head = 3: the base table computed the present way; the words in which the adopted one differed (one counter, zeroed when allocated)
    int64_t next_head_iterations = 0;  // iterations since the context was created whose base table was adopted
    DevBuf d_loop_extra;   // additional rows of the two batches: [1+P][a] | [9][a]
    DevBuf d_loop_iter;    // LoopFlags | IterResult[num_iter]
    DevBuf d_panel_work;   // scratch of the blocked device solve for P > 64 (published panels, inverse, hand-over flags)
    uint32_t panel_epoch = 0;
    int panel_P = -1;       // parameter count the scratch is laid out for
    DevBuf d_rot_same;     // per evaluation of the Jacobian batch: 1 = its control rotations are evaluation 0's bit for bit (pose-table kernels)
    DevBuf d_sync;         // counters of the device-side stream dependencies (dev_sync.h: SyncSlot), zeroed when the context is created
    int wait_seq = 0;                    // wait kernels enqueued by the current whole call (debug switch sync_fault withholds the signal of one of them)
    long long* stamp_voxel = nullptr;    // debug switch gap_stamps = 2: where build_gaussians stamps "voxelisation done" / "fit done"
    long long* stamp_fit = nullptr;
    int voxel_calls = 0;                 // voxelisations of the current whole call (debug switch speculation_fault plants a wrong guess in one of them)
    int small_voxel_launches = 0, small_voxel_fallbacks = 0;  // voxelisations on the one-launch path; voxelisations the small path (small_voxel.hip) handed back to the general path (codes wider than 32 bits)
    int sync_retries = 0, speculation_retries = 0;  // since the context was created: calls re-run with events after a wait timed out; voxelisations re-run after a wrong guess
    DevBuf d_aos_raw, d_aos_idx;         // include/dmsa_aos.h: the caller's strided clouds as they lie in memory, and their per-point indices
    DevBuf d_static_keep;                // the static points as uploaded (a call that has to start over restores them: centralize / decentralize is no exact round trip)
    DevBuf d_ctrl_pm, d_dT;              // analytic Jacobian: the 2P central-difference control-pose sets, the pose-table derivatives [rows][12][P]
    PinnedBuf h_results;  // IterResult per iteration
    // one extra device->host copy riding on the counts read-back of build_gaussians (the previous iteration's IterResult)
    const void* rb_extra_src = nullptr;
    void* rb_extra_dst = nullptr;
    size_t rb_extra_bytes = 0;
    int M = 0, M1 = 0;
    int64_t Mm = 0;
    bool gaussians_valid = false;
    // residual batches
    DevBuf d_E, d_ne_partial, d_Hp, d_sq_partial, d_sq_out;
    int64_t ldE = 0;
    int extra_rows = 0;
    // timing
    DevBuf d_batch_clock;          // batch stamps: ticks of all stamped batches since the context was created (one 64-bit word; a timed-out wait clears d_sync, not this)
    unsigned long long batch_ticks_seen = 0;  // ... of which t_ms[T_RESIDUAL] holds this many
    int wall_clock_khz = 0;        // hipDeviceAttributeWallClockRate
    bool batch_ticks_dirty = false, batch_ticks_in_flight = false;  // stamped batches enqueued since the last copy of [1]; that copy is on `stream`
    std::vector<EventPair> pending;
    std::vector<hipEvent_t> free_events;
    double t_ms[T_COUNT] = {0, 0, 0, 0, 0, 0};
    int64_t residual_launches = 0, residual_evals = 0;
    double residual_bytes = 0.0, residual_unit_bytes = 0.0;
    int evaluations = 0;
    std::vector<dmsa_iter_trace> trace;
    HostTimeline tl;
    StaticState* sp = nullptr;
    WorkerPool* pool = nullptr;  // created on first use
    struct PcdState* pcd = nullptr;  // scratch of the PCD export (pcd_export.cpp), created on first use
};

#define HIPCHK(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess) {                                                                               \
            ctx->err = std::string(#expr) + ": " + hipGetErrorString(_e);                                     \
            return DMSA_ERR_HIP;                                                                              \
        }                                                                                                     \
    } while (0)

#define CHK(expr)                  \
    do {                           \
        int _rc = (expr);          \
        if (_rc != DMSA_OK) return _rc; \
    } while (0)

inline int fail(dmsa_ctx* ctx, int rc, const std::string& why) { return ctx->err = why, rc; }  // a status with its reason

// ---- shared helpers (context.cpp) ----
WorkerPool& workers(dmsa_ctx* ctx);
hipEvent_t get_event(dmsa_ctx* ctx);
struct ScopedTimer {
    dmsa_ctx* ctx;
    EventPair ev;
    bool on;
    ScopedTimer(dmsa_ctx* c, int slot, bool by_stamps = false) : ctx(c) {
        // the correspondence kernel is always timed (roofline contract): by the device's clock inside its own kernels where run_residuals says
        // so (by_stamps), by this event pair otherwise; other stages only on request
        on = (slot == T_RESIDUAL || (c->flags & DMSA_FLAG_STAGE_TIMERS) != 0) && !by_stamps;
        if (!on) return;
        ev.a = get_event(c), ev.b = get_event(c), ev.slot = slot;
        (void)hipEventRecord(ev.a, c->stream);
    }
    ~ScopedTimer() {
        if (!on) return;
        (void)hipEventRecord(ev.b, ctx->stream);
        ctx->pending.push_back(ev);
    }
};
void drain_timers(dmsa_ctx* ctx);
// Batch stamps: in front of the synchronisation that ends a call, the copy of the tick accumulator (nothing if no stamped batch ran since the
// last one); drain_timers folds it into t_ms[T_RESIDUAL] behind that synchronisation.
hipError_t enqueue_batch_ticks(dmsa_ctx* ctx);
hipError_t sync_spin(hipStream_t stream);
int set_device(dmsa_ctx* ctx);
// Did a device-side wait of the call that just ended give up?  Synchronises the device, clears the flag and the counters (whatever the
// call's own status was: a stale flag or a half-counted signal must not reach the next call).  `what` receives the counter values.
bool sync_wait_timed_out(dmsa_ctx* ctx, std::string* what);
int num_params(const dmsa_ctx* ctx);
PoseChain& chain(dmsa_ctx* ctx);
int num_extra_rows(const dmsa_ctx* ctx);
int alloc_point_buffers(dmsa_ctx* ctx, int64_t n);  // everything whose size depends only on the point count `n`, the problem's own arrays apart
int upload_powm1_codes(dmsa_ctx* ctx, int64_t counts);
int upload_loop_model(dmsa_ctx* ctx, Model model);
void write_back_poses(const PoseChain& c, double* rel_o, double* rel_t);
// ---- upload_driver.cpp (the state rule of an upload is written at its top) ----
// The one place that sizes a problem's own arrays: d_local, d_ring and -- a window -- d_stamps / d_fhw / d_trajtime or -- with_normals, a keyframe problem -- d_nlocal / d_nglobal.
// While a problem is resident (a reservation) a block that moves keeps what it held.
int ensure_problem_buffers(dmsa_ctx* ctx, int64_t n, int rows, bool with_normals);
// dmsa_reserve and dmsa_window_ring_create: every buffer of a problem of n points, `rows` pose-table rows (identity row included) and P parameters.
// A resident problem keeps its sizes, its arrays and its global points; what else was derived from them (tables, Gaussians) is withdrawn, and
// a failure withdraws the problem itself.
int reserve_problem(dmsa_ctx* ctx, int64_t n, int rows, bool with_normals, int P);
int upload_begin(dmsa_ctx* ctx, const dmsa_window_problem* p, int64_t N, int64_t S);
int upload_begin(dmsa_ctx* ctx, const dmsa_keyframe_problem* p, int64_t n);
int upload_commit(dmsa_ctx* ctx, Model model);
// where the N moving points of a window come from ...
struct WindowPoints {
    enum Kind { FLAT, AOS, RING } kind;
    int64_t count;
    const dmsa_aos_view* clouds;  // AOS
    int32_t num_clouds;
    double t0;  // RING
    static WindowPoints flat(const dmsa_window_problem* p) { return {FLAT, p->num_points, nullptr, 0, 0.0}; }  // p's flat arrays, packed on the host
    static WindowPoints aos(const dmsa_aos_view* clouds, int32_t num_clouds, int64_t N) { return {AOS, N, clouds, num_clouds, 0.0}; }  // raw bytes, packed on the device
    static WindowPoints ring(int64_t N, double t0) { return {RING, N, nullptr, 0, t0}; }  // the resident ring, assembled on the device
};
// ... and its static tail: coordinates and ring ids at two strides
struct StaticPoints {
    int64_t count;
    const char *xyz, *id;
    size_t xyz_stride, id_stride;
    static StaticPoints flat(const dmsa_window_problem* p) {
        return {p->num_static, reinterpret_cast<const char*>(p->xyz_static), reinterpret_cast<const char*>(p->ring_id_static), 16, 4};
    }
    static StaticPoints aos(const dmsa_aos_view* v) {  // (null: none)
        if (!v) return {0, nullptr, nullptr, 0, 0};
        return {v->count, static_cast<const char*>(v->base) + v->xyz_offset, static_cast<const char*>(v->base) + v->aux_offset, (size_t)v->stride, (size_t)v->stride};
    }
};
int upload_window(dmsa_ctx* ctx, const dmsa_window_problem* p, const WindowPoints& pts, const StaticPoints& st);
int upload_keyframes(dmsa_ctx* ctx, const dmsa_keyframe_problem* p, int64_t n, const dmsa_aos_view* frames /* null: p's flat arrays */);
void copy_parallel(dmsa_ctx* ctx, char* dst, const char* src, size_t total);  // bytes [0, total) copied by the context's worker threads
// ---- window_ring.cpp ----
// The ring's own refusals, for both of its upload entries: `num_points` is what the problem says (0: nothing), *N the ring's resident points.
int ring_upload_checks(dmsa_ctx* ctx, float min_grid_size, int64_t num_points, bool static_arrays_ok, int64_t* N);
// ---- next_rows_api.cpp ----
// the message checks of dmsa_decode_pointcloud2: *n_out = points of the message (0: nothing else was looked at), *f_out = the byte offsets the sensor type reads
int pointcloud2_layout(const dmsa_pointcloud2* msg, int32_t sensor, PointCloud2Fields* f_out, uint64_t* n_out);
// the checks of a field descriptor against a message pointcloud2_layout has passed (include/dmsa_dense_intensity.h, I4): *offset_out = its byte offset in a point
int pointcloud2_field_layout(const dmsa_pointcloud2* msg, uint32_t index, uint32_t datatype, uint32_t* offset_out);
// ---- pcd_export.cpp ----
void pcd_release(dmsa_ctx* ctx);  // deletes ctx->pcd (dmsa_destroy)
// ---- voxelize_driver.cpp ----
// What a caller asks of build_gaussians besides the settings; the defaults are an everyday build.
struct BuildRequest {
    // (optional) runs on the host after every voxelisation kernel has been enqueued and before the counts are read back: host work placed there
    // hides behind the GPU
    std::function<int()> overlap;
    // (optional) the caller's enqueues for the third stream that belong in FRONT of the voxelisation's own (the device loop's chains and pose
    // tables of the Jacobian batch).  build_gaussians calls it once -- first of all in the common order, behind k_lattice when that runs on the
    // third stream (keys_ahead).
    std::function<int()> side_head;
    // what the build may try; its own redo (voxelize_driver.cpp) withdraws them one by one
    bool allow_speculation = true;  // sort widths from the previous voxelisation instead of sync #1
    bool allow_compression = true;  // leaf codes of only the bits that vary (debug switch key_compress)
    bool allow_small = true;        // the one-launch path for small clouds (debug switch small_voxel)
};
int build_gaussians(dmsa_ctx* ctx, const dmsa_settings& s, const BuildRequest& rq);
// ---- optimize_loop.cpp ----
int build_tables(dmsa_ctx* ctx, int B, const std::vector<double>& globs, hipStream_t stream = nullptr);
void append_glob(const PoseChain& c, std::vector<double>& out);
void host_set_params(dmsa_ctx* ctx, const double* p);
int transform_points(dmsa_ctx* ctx, int b);
int ensure_E(dmsa_ctx* ctx, int B);
int run_residuals(dmsa_ctx* ctx, int B, const std::vector<double>* extra, const double* d_extra = nullptr, const uint32_t* rot_same = nullptr,
                  const int2* row_range = nullptr /* Jacobian batch of the device loop: pairs equal to evaluation 0 are left out (serial_kernels.h) */);
int device_lm_step(dmsa_ctx* ctx, const double* d_Hp, int P, double lambda, double alpha, double max_step, double* d_step, LoopFlags* d_flags);
// ---- analytic Jacobian (settings.use_analytic_jacobi; optimize_loop.cpp) ----
constexpr double kTableDerivStep = 1e-5;  // central-difference step of the pose-table derivatives
int check_analytic_jacobian(dmsa_ctx* ctx, int P);  // DMSA_ERR_INVALID (with the reason) for a P the Jacobian kernel does not take
// d_dT <- the pose-table derivatives at the host chain's current parameters (2P chains on the host, tables on the device)
int host_table_derivatives(dmsa_ctx* ctx, hipStream_t stream);
// the additional rows of a batch of B evaluations (host vector, B x a) below the Gaussian rows of E
int upload_extra(dmsa_ctx* ctx, const std::vector<double>& extra, int B);
// E[1..P] <- [J | e0]: the additional rows' forward differences (E holds their 1 + P evaluations) and the Gaussian rows from d_dT and `table0`
int analytic_columns(dmsa_ctx* ctx, int P, double inv_h, const float* table0);
int optimize(dmsa_ctx* ctx, const dmsa_settings& s, dmsa_report* rep);
int adaptive_step_size(dmsa_ctx* ctx, double* params, const double* step, double error0, int32_t* best_k);
