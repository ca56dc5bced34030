// voxelize_driver.cpp — currentGauss.reset() + createGaussianSets at both resolutions + Gaussian fit + updateRebalancingWeights
// (DmsaOptimizer.h:78-96) as one launch sequence over three streams; kernels in dmsa_kernels.hip / radix_sort.hip / serial_kernels.hip.
//
// How to read this file: make_plan decides every mode of a build (VoxelPlan) before anything is enqueued, resolve_sort_widths adds the two values
// that may have to wait for sync #1, and the phases (members of VoxelBuild) read the plan and decide nothing.  common_order / by_level_order are
// the two launch sequences up to the read-back, build_gaussians is the spine: plan, lattice, one of the orders, sync #2, verdict, rest of the fit.
#include "dmsa_ctx.h"

// the fields of a lattice table that the key kernel or a kernel downstream of it reads: a voxelisation keyed with `a` is the one `b` gives iff they agree
static bool same_keying_table(const LatticeTable& a, const LatticeTable& b) {
    if (a.status != 0 || b.status != 0 || a.num_events != b.num_events || a.num_events < 0 || a.num_events > kMaxLatticeEvents) return false;
    if (a.defined != b.defined || a.first_idx != b.first_idx || a.final_depth != b.final_depth || a.compressed != b.compressed || a.total_bits != b.total_bits) return false;
    const size_t E = (size_t)a.num_events;
    return std::memcmp(a.event_idx, b.event_idx, E * sizeof(a.event_idx[0])) == 0 && std::memcmp(a.mn, b.mn, (E + 1) * sizeof(a.mn[0])) == 0 &&
           std::memcmp(a.suffix_shift, b.suffix_shift, (E + 1) * sizeof(a.suffix_shift[0])) == 0 && std::memcmp(a.depth, b.depth, (E + 1) * sizeof(a.depth[0])) == 0 &&
           std::memcmp(a.final_mn, b.final_mn, sizeof(a.final_mn)) == 0 && std::memcmp(a.nbits, b.nbits, sizeof(a.nbits)) == 0 &&
           std::memcmp(a.key_base, b.key_base, sizeof(a.key_base)) == 0;
}

namespace {

// Rule of keys_ahead = 1: only behind kKeysAheadStreak consecutive voxelisations of the context whose tables did not change (the host compares
// each read-back set with the one before; an upload and a redo start the count again).  A redo costs a whole voxelisation (~250 us on the
// bench window) where the ahead order saves ~21 us, so it pays below one redo in about twelve builds; the first iterations on a new cloud
// are far above that (the 140 000-point rosette window: 5 redos in its first 25 iterations, none in the 180 behind them, and 20-step runs
// 3 % below the parent with the rule "wherever possible"), the converged ones far below.  8 is a guess between those, not a measured optimum.
// The device copy of the set is made only when the next build may use it.
constexpr int kKeysAheadStreak = 8;

// ---- The plan: every decision of one build ------------------------------------------------------------------
struct VoxelPlan {
    // -- make_plan: from the context, the settings and the request, before anything is enqueued --
    int64_t n;
    int aabb_blocks;      // blocks of launch_block_aabb, which k_lattice reduces
    bool lvl_on[2];       // a disabled level is keyed with the other level's lattice (level_res is aliased) and ignored later
    bool compress;        // leaf codes hold only the bits that vary over the points
    bool small;           // the one-launch path (small_voxel.hip)
    bool speculate;       // sort widths from the previous voxelisation: no sync #1
    bool prehist;         // the key kernels count the digits of the sort that follows
    bool two;             // level 1 on a stream of its own
    bool by_level;        // by_level_order instead of common_order
    bool split;           // splitSet of the keyframe pass: two slots per leaf
    bool ahead_possible;  // the switches and the size allow the ahead order at all (hand_over_tables keeps the keying set for the next build)
    bool ahead;           // keys and sorts on the keying set, k_lattice beside them on the third stream
    bool merged;          // both levels in one sort of 2n pairs
    hipStream_t st[2];    // the stream of each level
    hipStream_t rb;       // the stream of the read-back
    LatticeTable* key_tab;  // [2]: the tables every kernel behind k_lattice reads
    int items;            // tile choice of the sorts: the sort plans and the sorts they describe are given the same one
    int small_threshold;  // size classes: Gaussians up to this many members walk them on one lane group
    // -- resolve_sort_widths: behind the lattice launch (not speculating: behind sync #1) --
    int sort_depth[2], sort_bits[2];
    int tag_bit;          // level 1's tag in a merged sort; bit `sort_bits` is the marker of non-finite points
    unsigned end_bit;     // of the merged sort
    bool k32;             // 32-bit leaf codes (both levels share the width: they may be sorted together)
    bool prepared;        // the sorts find header, look-back state and histograms done (prehist with 32-bit codes)
    SortPlan sort_plan[2];  // merged: one sort of 2n pairs in workspace 0, both key kernels count into its header
};

VoxelPlan make_plan(const dmsa_ctx* ctx, const dmsa_settings& s, const BuildRequest& rq) {
    const VoxelState& v = ctx->vox;
    const int64_t n = ctx->n;
    VoxelPlan p{};
    p.n = n;
    p.aabb_blocks = (int)((n + kAabbBlock - 1) / kAabbBlock);
    p.lvl_on[0] = s.grid_size_1_factor > std::numeric_limits<float>::min(), p.lvl_on[1] = s.grid_size_2_factor > std::numeric_limits<float>::min();
    p.compress = ctx->dbg.key_compress != 0 && rq.allow_compression;
    p.split = s.gauss_split != 0 && ctx->model == MODEL_KEYFRAMES;
    // The reference's everyday size (5 scans x <= 3000 points + static points): ONE launch from the lattice to the member lists, a workgroup per
    // resolution (small_voxel.hip).  The kernel takes the tree depths and code widths from the lattice table on the device: nothing to
    // speculate on, no second stream, no joins.  Codes wider than 32 bits make it give up (counts.pad) and the general path runs.
    p.small = rq.allow_small && ctx->dbg.small_voxel != 0 && n <= small_voxel_max_points() && p.lvl_on[0] && p.lvl_on[1] && !p.split && ctx->dbg.voxel_coherence == 0;
    // The sort only needs an UPPER bound of the tree depth.  From the second iteration on the previous depths are used
    // without waiting for the lattice kernel; the true depths arrive with the counts (sync #2) and a too-small guess (the
    // bounding box doubled between two iterations) re-runs the voxelisation synchronously.
    p.speculate = p.small || (rq.allow_speculation && v.depth_guess[0] >= 0 && v.depth_guess[1] >= 0 && v.depth_guess[0] < 20 && v.depth_guess[1] < 20 &&
                              (!p.compress || (v.bits_guess[0] >= 0 && v.bits_guess[1] >= 0)));
    // the key kernels count the digits of the sort that follows (own sort, 32-bit codes): no clearing kernel, no histogram pass
    p.prehist = ctx->dbg.sort_prehist != 0;
    // The two resolutions are independent until their member lists are appended (level 1 starts at level 0's totals):
    // level 0 runs on `stream`, level 1 on `stream2`; their launches are enqueued stage by stage so that both streams fill.
    p.two = ctx->dbg.dual_stream != 0 && p.lvl_on[0] && p.lvl_on[1];
    p.st[0] = ctx->stream, p.st[1] = p.two ? ctx->stream2 : ctx->stream;
    // The read-back of the counts runs on the third stream: a device-to-host copy ends with a system-scope release that holds up the
    // stream it is on for ~20 us, and the fit behind it does not need to wait for that.
    p.rb = ctx->dbg.dual_stream != 0 ? ctx->stream3 : ctx->stream;
    // Each level's size classes, gather and fit behind its own leaf scan (debug switch fit_by_level; by_level_order).  The sizes come
    // from k_leaf_finalize, so the single-workgroup scan and the one-launch path keep the common order.
    // 1 (default) goes by size, like small_threshold: windows of a few ten thousand points are bound by the host's launches, and this order has more of
    // them (the 25 360-point IMU window: 3686-3817 against 4027-4063 it/s); 2: whatever the size.  The 200 000 is a guess between the measured points,
    // not a measured crossover: slower at 25 360 points, 1-3 % faster at the 140 000-point rosette window (which the rule leaves out), at the
    // keyframe pass and at 1.5 M points.
    p.by_level = (ctx->dbg.fit_by_level >= 2 || (ctx->dbg.fit_by_level == 1 && n >= 200000)) && p.two && !p.small && ctx->dbg.fused_leaf_scan != 0;
    // ---- Keys ahead of the lattice (debug switch keys_ahead) ----
    // k_lattice is two workgroups and 22 us alone on the main stream, and in 98 % of a window's iterations all it does is prove that the tables the
    // previous voxelisation left are, bit for bit, the ones a replay would give.  In the AHEAD order nobody waits for that proof: the key kernel and
    // the sort of each level follow the transform directly and read the KEYING set (ctx->d_keying, the previous voxelisation's tables), and so does
    // every later kernel that takes a table; k_lattice runs beside them on the third stream, takes its hint from the keying set and writes this
    // cloud's tables into d_lattice, which the host reads back with the counts as ever.  At sync #2 the host compares the two sets
    // (same_keying_table): equal in every field a kernel read, the voxelisation is the one the common order gives; otherwise it is redone in the
    // common order, like a mis-speculated sort width.  Nothing writes the keying set while a kernel can read it: k_lattice only reads it, the key
    // kernel reports a key outside the compressed range in GaussCounts::pad[2] (cleared with the counts by the transform) and writes only code_or,
    // the same value from launch to launch, and the set is refreshed by a copy on the main stream behind a voxelisation in the common order, with
    // nothing of a voxelisation in flight.  The sort headers that k_lattice clears in the common order are cleared by the first workgroup of the key
    // kernel on the sort's own stream (not with sort_prehist, whose key kernels add to the header from every workgroup: common order).
    // Downstream of keys made from a stale table: such keys are the keys of an earlier, accepted voxelisation's table applied to other coordinates
    // -- masked to depth[e] bits per axis plus that table's shifts, or the low nbits per axis: below the table's invalid code whatever the point --
    // and the guessed sort width is that table's (depth_guess / bits_guess are taken from the tables that become the keying set; a compression flag
    // that changed in between keeps the common order).  The sorts move (key, index) pairs of indices 0 .. n - 1 and look at no bit at or above their
    // end bit; k_leaf_segments / k_head_flags / k_leaf_starts compare neighbouring codes with each other and with the table's invalid code and count
    // at most n leaves; k_leaf_accept, k_leaf_split, k_leaf_finalize and k_gather_members index by position, leaf and slot, all bounded by n (2n
    // slots), and read points through the sorted indices; the size classes and the fit are sized by Gaussians <= 2n + 16.  None of them looks at a
    // coordinate to form an address, so a wrong table gives wrong leaves, never an index out of range -- what a too-narrow speculated sort, which
    // merges leaves arbitrarily, has fed them since round 2.
    // The build behind a redo runs in the common order (keying_valid is cleared): what moved a trigger or the range is likely to move it again.
    // (also left to the common order: one stream for everything, and stage timers, whose event pairs would bracket other streams' kernels)
    p.ahead_possible = ctx->dbg.keys_ahead != 0 && ctx->dbg.dual_stream != 0 && ctx->dbg.lattice_hint != 0 && !p.prehist && !p.small && n > 0 &&
                       (ctx->flags & DMSA_FLAG_STAGE_TIMERS) == 0;
    if (p.ahead_possible && p.speculate && v.lattice_hint_valid && v.keying_valid && v.keying_n == n) {
        // Codes of either width: the width follows the guess in both orders, and a sort of 64-bit codes clears its own header.  (The window of
        // the bench has 32-bit codes; the near-miss clouds of the tests, whose far outlier makes a box of depth 13, have 38-bit ones.)
        p.ahead = true;
        for (int l = 0; l < 2; ++l) p.ahead = p.ahead && v.h_keying[l].compressed == (p.compress ? 1 : 0);
    }
    p.key_tab = p.ahead ? ctx->d_keying.as<LatticeTable>() : ctx->d_lattice.as<LatticeTable>();
    // Small clouds (keyframe sets: 3 x 10^5 points) are launch-bound: one sort of 2n pairs on one stream.  Large clouds (the window:
    // 1.5 x 10^6) keep the two levels on two streams with one sort each (a sort only looks at the bits below its end bit, so the
    // tag is inert there).
    p.merged = ctx->dbg.merge_sort < 0 ? n <= (int64_t)(1 << 20) : ctx->dbg.merge_sort != 0;
    p.items = ctx->dbg.sort_items;
    // Which Gaussians walk their members on one lane group (k_residuals_small, the fit's one-wave class) and which get a workgroup
    // (chain tiers, the fit's four-wave class)?  The lane-per-evaluation kernel spends the fewest instructions per member, but a wave of
    // it walks up to `threshold` members one after the other: with a few thousand Gaussians (the reference's everyday windows, small
    // keyframe sets) its few hundred waves leave the chip idle while the longest of them runs.  Measured (it/s at thresholds 8 = nobody /
    // 32 / 256, scripts/threshold_ab.sh): config-2 window, 1100 Gaussians 3450 / 3090 / 2580; 8 keyframes, 2465: 1965 / 1955 / 1906;
    // 12 keyframes, 3823: 1672 / 1782 / 1726; 16 keyframes, 4920: 1353 / 1534 / 1502; 24 keyframes, 6906: 910 / 1080 / 1213; the bench
    // window, 13 000: - / 1196 (64) / 1262.  Every tier computes the same bits, so the rule may follow the size of the previous
    // voxelisation (the first one of a context goes by the number of points).
    // (build_gaussians has cleared ctx->M by the time the plan is made, so as things stand the rule always goes by the number of points.)
    const int auto_threshold = ctx->M > 0 ? (ctx->M < 2000 ? 8 : ctx->M < 6000 ? 32 : 0) : (n < 60000 ? 8 : n < 200000 ? 32 : 0);
    p.small_threshold = ctx->dbg.small_threshold > 0 ? ctx->dbg.small_threshold : auto_threshold;
    return p;
}

// The second step of the plan, behind the lattice launch: the widths of the sorts -- the previous voxelisation's when speculating (the true ones
// arrive with the counts, sync #2), else the ones sync #1 has just brought -- and what follows from them: the code width, the level views into
// the shared code / index arrays, the sort plans.
int resolve_sort_widths(dmsa_ctx* ctx, VoxelPlan& p) {
    const VoxelState& v = ctx->vox;
    const int64_t n = p.n;
    for (int l = 0; l < 2; ++l) {
        p.sort_depth[l] = p.speculate ? v.depth_guess[l] : ctx->h_lattice[l].final_depth;
        // width of the leaf codes: all 3*depth bits, or (compressed) only the bits that vary over the points
        p.sort_bits[l] = !p.compress ? 3 * p.sort_depth[l] : (p.speculate ? v.bits_guess[l] : ctx->h_lattice[l].total_bits);
        if (!p.speculate && p.lvl_on[l] && ctx->h_lattice[l].status != 0) return ctx->h_lattice[l].status;
    }
    // Both resolutions are keyed into one array of 2n (code, point) pairs -- level 1 carries a tag bit above the widest code --
    // and sorted by ONE radix sort: half the launches, twice the parallelism per pass, and the sorted halves are the two levels.
    if (ctx->dbg.trace_time >= 3) std::fprintf(stderr, "[voxelize] key bits (without the marker of non-finite points): level 0 %d, level 1 %d\n", p.sort_bits[0], p.sort_bits[1]);
    p.tag_bit = std::max(p.sort_bits[0], p.sort_bits[1]) + 1;  // bit `sort_bits` is the marker of non-finite points
    p.end_bit = (unsigned)(p.tag_bit + 1);
    p.k32 = p.small || p.end_bit <= 32;  // (the small path writes 32-bit codes or gives up)
    const size_t ksz = p.k32 ? 4 : 8;
    for (int l = 0; l < 2; ++l) {
        ctx->key32[l] = p.k32;
        ctx->code_v[l] = ctx->d_code[0].as<char>() + (size_t)l * n * ksz, ctx->code_s_v[l] = ctx->d_code_s[0].as<char>() + (size_t)l * n * ksz;
        ctx->idx_v[l] = ctx->d_idx[0].as<uint32_t>() + (size_t)l * n, ctx->idx_s_v[l] = ctx->d_idx_s[0].as<uint32_t>() + (size_t)l * n;
    }
    p.prepared = p.prehist && p.k32;
    for (int l = 0; l < 2 && !p.small; ++l)
        p.sort_plan[l] = p.merged ? sort_pairs_u32_plan(ctx->d_sort_tmp[0].p, (size_t)(2 * n), p.end_bit, p.items)
                                  : sort_pairs_u32_plan(ctx->d_sort_tmp[l].p, (size_t)n, (unsigned)(p.sort_bits[l] + 1), p.items);
    return DMSA_OK;
}

// why a voxelisation is run again (VoxelBuild::redo)
enum class Redo { SmallGaveUp, TablesMoved, KeyLeftRange, SortTooNarrow };

// ---- One build: the phases --------------------------------------------------------------------------------------
// Each phase enqueues what its name says, on the streams the plan names, and decides no mode.  What one phase leaves for a later one (a signal
// still to be carried, the grids of the speculated fit) is a member below the plan.
struct VoxelBuild {
    dmsa_ctx* const ctx;
    const dmsa_settings& s;
    const BuildRequest& rq;
    const VoxelPlan& p;
    // device addresses every phase shares
    GaussCounts* const counts;
    SerialCounts* const d_serial;      // merged | level 0 | level 1
    int32_t* const gsize[2];           // fit_by_level: members of every Gaussian of a level (k_leaf_finalize)
    uint32_t* const order_level[2];    // ... and the Gaussians of each level by descending size class
    StreamDep* const sizes_dep[2];
    StreamDep* const classes_dep[2];
    const float* const fit_table;
    // from phase to phase
    uint32_t* lattice_signal = nullptr;  // k_lattice carries the signal for level 1's stream (dev_sync.h), one per resolution
    uint32_t* ahead_signal = nullptr;    // ahead: "the transform is through", given by the first key kernel of the main stream as it starts
    int fit_launched[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // [level; 2 = merged][class]: grids of the speculated fit
    int finish_launched = 0;
    bool weights_launched = false;
    GaussCounts h{};  // the counts as sync #2 brought them (verdict)

    VoxelBuild(dmsa_ctx* c, const dmsa_settings& settings, const BuildRequest& request, const VoxelPlan& plan)
        : ctx(c), s(settings), rq(request), p(plan), counts(c->d_counts.as<GaussCounts>()),
          d_serial(reinterpret_cast<SerialCounts*>(c->d_counts.as<char>() + sizeof(GaussCounts))),
          gsize{c->d_gauss_size[0].as<int32_t>(), c->d_gauss_size[1].as<int32_t>()},
          order_level{c->d_order_level.as<uint32_t>(), c->d_order_level.as<uint32_t>() + plan.n + 8}, sizes_dep{&c->sizes0, &c->sizes1},
          classes_dep{&c->classes0, &c->classes1}, fit_table(c->base_table ? c->base_table : c->d_tables.as<float>()) {}

    // ---- lattice ----
    // k_lattice, stated once: on `stream`, carrying `signal`, clearing the two sort headers on the side, with the hint read from `hint_src`
    // (null: from d_lattice itself)
    void launch_lattice_on(hipStream_t stream, uint32_t* signal, void* header0, void* header1, const LatticeTable* hint_src, bool use_hint) {
        launch_lattice(ctx->d_global.as<float4>(), p.n, ctx->d_aabb.as<float>(), p.aabb_blocks, ctx->level_res[0], ctx->level_res[1], p.compress,
                       ctx->d_lattice.as<LatticeTable>(), header0, header1, stream, signal, use_hint, hint_src);
    }
    // the block bounds, k_lattice on the main stream (not ahead) and, when not speculating, sync #1
    int lattice_main() {
        ScopedTimer tm(ctx, T_VOXEL);
        if (!ctx->aabb_fresh)  // the device loop's fused transform already left the block bounds and cleared the counters
            launch_block_aabb(ctx->d_global.as<float4>(), p.n, ctx->d_aabb.as<float>(), ctx->d_counts.p, sizeof(GaussCounts) + sizeof(SerialCounts),
                              ctx->stream);
        ctx->aabb_fresh = false;
        // the lattice kernel clears the headers of the own radix sorts on the side (one dispatch less per sort)
        if (!p.small && !p.ahead) lattice_signal = ctx->lattice.kernel_signal(ctx->stream, p.st[1], 2);
        if (!p.ahead)  // (ahead: on the third stream, behind the first key kernel's launch -- lattice_aside)
            launch_lattice_on(ctx->stream, lattice_signal, ctx->d_sort_tmp[0].p, ctx->d_sort_tmp[1].p, nullptr,
                              ctx->dbg.lattice_hint != 0 && ctx->vox.lattice_hint_valid);
        ctx->vox.lattice_hint_valid = true;  // (a table of another problem is harmless: it fails the verification and the replay runs)
        if (!p.speculate) {  // sync #1: tree depths select the radix-sort bit range (speculation reads them with the counts instead)
            HIPCHK(hipMemcpyAsync(ctx->h_lattice, ctx->d_lattice.p, 2 * sizeof(LatticeTable), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(sync_spin(ctx->stream));
        }
        return DMSA_OK;
    }
    // k_lattice of the ahead order: on the third stream, as soon as the transform is through, in front of whatever the caller has for that stream
    int lattice_aside() {
        CHK(ctx->lattice.wait(ctx->stream3, ctx->stream));
        launch_lattice_on(ctx->stream3, nullptr, nullptr, nullptr, p.key_tab, true);
        if (rq.side_head) CHK(rq.side_head());
        return DMSA_OK;
    }
    // scratch of splitSet (keyframe pass)
    int split_scratch() {
        if (p.split && !ctx->d_split_stats.p) {
            HIPCHK(ctx->d_split_stats.ensure(64 * 16));  // 64 stripes of (blocks looked at, blocks skipped)
            HIPCHK(hipMemsetAsync(ctx->d_split_stats.p, 0, 64 * 16, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));  // (both level streams add to it)
        }
        if (p.split)
            for (int l = 0; l < 2; ++l) {
                HIPCHK(ctx->d_pos_slot_rank[l].ensure((size_t)p.n * 4));
                HIPCHK(ctx->d_nsorted[l].ensure((size_t)p.n * 16));
                HIPCHK(ctx->d_pair_d[l].ensure(split_scratch_bytes(p.n)));
            }
        return DMSA_OK;
    }

    // ---- keys and sorts ----
    void keys(int l, hipStream_t stream) {  // a disabled level is keyed with the other level's lattice (level_res is aliased) and ignored later
        const int64_t n = p.n;
        SortPlan pl = p.sort_plan[l];
        if (p.merged && l == 1) pl.state_words = 0;  // the look-back words of the common sort are cleared once
        VoxelKeysAhead ka;
        if (p.ahead) {
            ka.range_flag = &counts->pad[2];
            if (p.k32 && !(p.merged && l == 1)) ka.clear_header = reinterpret_cast<uint32_t*>(p.sort_plan[l].header);
            if (stream == ctx->stream) ka.start_signal = ahead_signal, ahead_signal = nullptr;
        }
        launch_voxel_keys(ctx->d_global.as<float4>(), n, p.key_tab + l, ctx->level_res[l], ctx->code_v[l], p.k32, ctx->idx_v[l],
                          l == 0 ? 0ull : (1ull << p.tag_bit), p.prepared ? &pl : nullptr, stream, ka);
        if (ctx->dbg.voxel_coherence != 0 && p.lvl_on[l]) {  // how many points changed leaf since the previous voxelisation of this context
            const size_t ksz = p.k32 ? 4 : 8;
            const bool compare = ctx->coh_valid[l] && ctx->d_code_prev[l].cap >= (size_t)n * ksz && ctx->coh_key32[l] == p.k32 && ctx->coh_n[l] == n;
            if (ctx->d_code_prev[l].ensure((size_t)n * ksz) != hipSuccess || ctx->d_coh_count.ensure(8) != hipSuccess) return;
            if (!ctx->coh_count_zeroed) (void)hipMemsetAsync(ctx->d_coh_count.p, 0, 8, stream), ctx->coh_count_zeroed = true;
            launch_count_code_changes(ctx->code_v[l], ctx->d_code_prev[l].p, p.k32, n, compare, ctx->d_coh_count.as<unsigned long long>(), stream);
            if (compare) ctx->coh_compared += n;
            ctx->coh_pending[l] = compare;
            ctx->coh_valid[l] = true, ctx->coh_key32[l] = p.k32, ctx->coh_n[l] = n;
        }
    }
    // the sort dispatch, stated once: `count` pairs of level `l`'s arrays (merged: both levels', from level 0's) in workspace `ws`, bits below `end_bit`
    int sort_pairs(const DevBuf& ws, int l, size_t count, unsigned end_bit, hipStream_t stream) {
        if (p.k32 && p.prepared)
            HIPCHK(sort_pairs_u32_onesweep(ws.p, ws.cap, (const uint32_t*)ctx->code_v[l], (uint32_t*)ctx->code_s_v[l], ctx->idx_v[l], ctx->idx_s_v[l], count, end_bit,
                                           p.items, stream, 2));
        else if (p.k32)
            HIPCHK(sort_pairs_u32_u32(ws.p, ws.cap, (const uint32_t*)ctx->code_v[l], (uint32_t*)ctx->code_s_v[l], ctx->idx_v[l], ctx->idx_s_v[l], count, end_bit,
                                      p.items, stream, true /* the lattice kernel (ahead: the key kernel) cleared the header */));
        else
            HIPCHK(sort_pairs_u64_u32(ws.p, ws.cap, (const uint64_t*)ctx->code_v[l], (uint64_t*)ctx->code_s_v[l], ctx->idx_v[l], ctx->idx_s_v[l], count, end_bit,
                                      p.items, stream));
        return DMSA_OK;
    }
    int keys_and_sort_both() {  // merged: on the main stream
        keys(0, ctx->stream), keys(1, ctx->stream);
        return sort_pairs(ctx->d_sort_tmp[0], 0, (size_t)(2 * p.n), p.end_bit, ctx->stream);
    }
    int keys_and_sort(int l) {  // one level on its stream
        keys(l, p.st[l]);
        return sort_pairs(ctx->d_sort_tmp[l], l, (size_t)p.n, (unsigned)(p.sort_bits[l] + 1), p.st[l]);
    }
    // keys and sorts of both levels, with the lattice dependency of level 1's stream and (ahead) k_lattice aside
    int keys_and_sorts() {
        if (p.ahead) {
            // The first key kernel of the main stream says, as it starts, that the transform is through (events: recorded in front of it); the waits
            // of the other two streams are enqueued behind the main stream's own kernels -- a wait enqueued ahead of them has its queue served
            // first and they start late (the measured rule below).
            ahead_signal = ctx->lattice.kernel_signal(ctx->stream, ctx->stream3);
            if (!ahead_signal) CHK(ctx->lattice.signal(ctx->stream, ctx->stream3));
        }
        if (p.merged) CHK(keys_and_sort_both());
        if (p.ahead && p.merged) CHK(lattice_aside());  // (before the signal behind the common sort is counted: this wait is for the key kernel's alone)
        // level 1 on its own stream: it needs the lattice (k_lattice signalled; ahead: the transform) and, merged, the common sort (a signal behind it;
        // with events the one signal)
        if (p.merged || (!p.ahead && !lattice_signal)) CHK(ctx->lattice.signal(ctx->stream, p.st[1]));
        if (!p.merged && p.ahead) {
            bool waited = false;  // the main stream's level first: its key kernel carries the signal
            for (int l = 0; l < 2; ++l)
                if (p.lvl_on[l] && p.st[l] == ctx->stream) CHK(keys_and_sort(l));
            for (int l = 0; l < 2; ++l)
                if (p.lvl_on[l] && p.st[l] != ctx->stream) {
                    if (!waited) CHK(ctx->lattice.wait(p.st[l], ctx->stream));
                    waited = true;
                    CHK(keys_and_sort(l));
                }
            CHK(lattice_aside());
        } else {
            CHK(ctx->lattice.wait(p.st[1], ctx->stream));
            if (!p.merged)
                for (int l = 0; l < 2; ++l)
                    if (p.lvl_on[l]) CHK(keys_and_sort(l));
        }
        return DMSA_OK;
    }

    // ---- leaves ----
    int leaves(int l) {
        const int64_t n = p.n;
        const LatticeTable* tab = p.key_tab + l;
        hipStream_t st = p.st[l];
        if (ctx->dbg.fused_segments != 0) {
            // one single-pass kernel; its look-back state is never cleared (epoch-tagged words, running ticket counter)
            ChainedScanCall call;
            HIPCHK(ctx->seg_state[l].begin((size_t)leaf_segment_tiles(n), kLeafSegmentWords, st, &call));
            launch_leaf_segments(ctx->code_s_v[l], p.k32, n, tab, ctx->d_leaf_incl[l].as<int32_t>(), ctx->d_leaf_start[l].as<int32_t>(), &counts->level[l], call, st);
        } else {
            launch_head_flags(ctx->code_s_v[l], p.k32, n, tab, ctx->d_head[l].as<int32_t>(), st);
            HIPCHK(inclusive_scan_i32(ctx->d_scan_tmp[l].p, ctx->d_scan_tmp[l].cap, ctx->d_head[l].as<int32_t>(), ctx->d_leaf_incl[l].as<int32_t>(), (size_t)n, st));
            launch_leaf_starts(ctx->d_head[l].as<int32_t>(), ctx->d_leaf_incl[l].as<int32_t>(), ctx->code_s_v[l], p.k32, tab, n,
                               ctx->d_leaf_start[l].as<int32_t>(), &counts->level[l], st);
        }
        launch_leaf_accept(ctx->d_leaf_start[l].as<int32_t>(), ctx->idx_s_v[l], ctx->d_ring.as<int32_t>(), &counts->level[l],
                           s.min_num_points_per_set, n, ctx->d_slot_acc[l].as<int32_t>(), ctx->d_slot_cnt[l].as<int32_t>(), st);
        if (p.split)
            launch_leaf_split(ctx->d_leaf_incl[l].as<int32_t>(), ctx->d_leaf_start[l].as<int32_t>(), ctx->idx_s_v[l], ctx->d_ring.as<int32_t>(),
                              ctx->d_nglobal.as<float4>(), &counts->level[l], s.min_num_points_per_set, n, ctx->d_nsorted[l].as<float4>(),
                              ctx->d_pair_d[l].as<unsigned long long>(), ctx->d_slot_acc[l].as<int32_t>(), ctx->d_slot_cnt[l].as<int32_t>(),
                              ctx->d_pos_slot_rank[l].as<int32_t>(), st, ctx->dbg.skip_stats != 0 ? ctx->d_split_stats.as<unsigned long long>() : nullptr);
        // slot scans: one multi-workgroup single-pass kernel (debug switch fused_leaf_scan = 0: the single-workgroup k_leaf_scan)
        if (ctx->dbg.fused_leaf_scan != 0) {
            ChainedScanCall call;
            HIPCHK(ctx->fin_state[l].begin((size_t)leaf_finalize_tiles(n), kLeafFinalizeWords, st, &call));
            launch_leaf_finalize(ctx->d_slot_acc[l].as<int32_t>(), ctx->d_slot_cnt[l].as<int32_t>(), n, ctx->d_gauss_of_slot[l].as<int32_t>(),
                                 ctx->d_memb_of_slot[l].as<int32_t>(), &counts->level[l], call, st, p.by_level ? gsize[l] : nullptr);
        } else
            launch_leaf_scan(ctx->d_slot_acc[l].as<int32_t>(), ctx->d_slot_cnt[l].as<int32_t>(), ctx->d_gauss_of_slot[l].as<int32_t>(), ctx->d_memb_of_slot[l].as<int32_t>(),
                             &counts->level[l], st);
        return DMSA_OK;
    }
    // (Enqueueing level 1 first -- its chain ends last -- was measured in round 5: 1089 instead of 1259 it/s.  Level 1's first kernel sits behind
    // a device-side wait; launched ahead of level 0's kernels the wait's queue is served first and level 0 starts late.
    // Swapping the streams as well -- level 1 on the main stream and enqueued first, level 0 behind the wait on the side stream -- was also
    // measured: 1243 against 1263 it/s on the headline window, the small windows and the keyframe set unchanged.)
    int leaves_of_both() {
        for (int l = 0; l < 2; ++l) {
            if (!p.lvl_on[l]) continue;
            CHK(leaves(l));
        }
        return DMSA_OK;
    }

    // ---- gathers ----
    void gather(int l, hipStream_t gs, uint32_t* start_signal = nullptr) {
        launch_gather_members(ctx->d_leaf_incl[l].as<int32_t>(), ctx->d_leaf_start[l].as<int32_t>(), ctx->idx_s_v[l],
                              ctx->code_s_v[l], p.k32, p.key_tab + l, ctx->d_slot_acc[l].as<int32_t>(), ctx->d_gauss_of_slot[l].as<int32_t>(),
                              ctx->d_memb_of_slot[l].as<int32_t>(), p.split ? ctx->d_pos_slot_rank[l].as<int32_t>() : nullptr, ctx->d_local.as<float4>(),
                              ctx->d_slot_cnt[l].as<int32_t>(), counts, l, p.n, ctx->d_memb_local.as<float4>(), ctx->d_memb_idx.as<int32_t>(),
                              ctx->d_memb_g.as<int32_t>(), ctx->d_seg_off.as<int32_t>(), gs, start_signal);
    }
    // Common order: both gathers on the first stream (level 1 appends behind level 0's totals anyway): the level-1 chain ends with its leaf scan,
    // long before level 0's gather is through, so the wait below finds its event signalled -- a join at the END of a stream costs
    // ~20 us of cross-queue signalling in front of everything that follows.
    int gathers_common() {
        CHK(ctx->level1.signal(p.st[1], ctx->stream));
        if (p.lvl_on[0]) gather(0, ctx->stream);
        CHK(ctx->level1.wait(ctx->stream, p.st[1]));
        if (p.lvl_on[1]) gather(1, ctx->stream);
        return DMSA_OK;
    }
    // By level: the kernel behind a level's k_leaf_finalize says that the sizes and totals of the level are final (its size classes on the
    // third stream may run) -- level 0's gather as it starts; on level 1's stream the one-wave wait for level 0's totals, behind which
    // level 1's members are appended (they are known long before: the wait finds them there), once it is through: level 1's Gaussians are
    // numbered behind level 0's, so its signal stands for both levels.
    int gathers_by_level() {
        uint32_t* sig = ctx->sizes0.kernel_signal(p.st[0], ctx->stream3);
        if (!sig) CHK(ctx->sizes0.signal(p.st[0], ctx->stream3));
        gather(0, p.st[0], sig);
        WaitCarry carry;
        carry.pass_on = ctx->sizes1.kernel_signal(p.st[1], ctx->stream3);
        CHK(ctx->sizes0.wait(p.st[1], p.st[0], 0, &carry));
        if (!carry.pass_on) CHK(ctx->sizes1.signal(p.st[1], ctx->stream3));  // (events: recorded behind the wait)
        gather(1, p.st[1]);
        return DMSA_OK;
    }

    // ---- the one-launch path: lattice tables to member lists in one kernel ----
    int small_path() {
        ScopedTimer tm(ctx, T_VOXEL);
        SmallVoxelArgs a{};
        a.global = ctx->d_global.as<float4>(), a.local = ctx->d_local.as<float4>(), a.ring = ctx->d_ring.as<int32_t>();
        a.n = (int)p.n, a.min_pts = s.min_num_points_per_set;
        a.tables = ctx->d_lattice.as<LatticeTable>();
        for (int l = 0; l < 2; ++l) {
            a.res[l] = ctx->level_res[l];
            a.code[l] = (uint32_t*)ctx->code_v[l], a.idx[l] = ctx->idx_v[l], a.code_s[l] = (uint32_t*)ctx->code_s_v[l], a.idx_s[l] = ctx->idx_s_v[l];
        }
        a.counts = counts;
        a.memb_local = ctx->d_memb_local.as<float4>(), a.memb_idx = ctx->d_memb_idx.as<int32_t>(), a.memb_g = ctx->d_memb_g.as<int32_t>();
        a.seg_off = ctx->d_seg_off.as<int32_t>();
        ctx->small_l0.inside_kernel(&a.sync, &a.sync_target, &a.timed_out);
        if (ctx->dbg.gap_stamps == 3) {  // phase stamps of the kernel (device wall clock, 100 MHz), printed after the counts have arrived
            HIPCHK(ctx->d_sv_stamps.ensure(2 * 16 * 8));
            a.stamps = ctx->d_sv_stamps.as<long long>();
        }
        launch_voxel_small(a, ctx->stream);
        ctx->small_voxel_launches += 1;
        HIPCHK(hipGetLastError());
        return DMSA_OK;
    }

    // ---- size classes and read-back ----
    // Common order: the size classes of the correspondence kernels need only seg_off, so they run before the read-back.
    // k_size_classes is one workgroup on the main stream between the voxelisation and the fit: it also carries two stream dependencies
    // (dev_sync.h) -- it waits for the pose tables of the Jacobian batch (built on the side stream long ago) and releases the read-back
    void size_classes_common() {
        DevSync sy;
        ctx->tables.kernel_wait_owed(sy);
        sy.signal_counter = ctx->classes.kernel_signal(ctx->stream, p.rb);
        launch_size_classes(ctx->d_seg_off.as<int32_t>(), counts, ctx->d_order.as<uint32_t>(), d_serial, ctx->stream, sy, p.small_threshold, ctx->dbg.long_log2);
    }
    // By level, all on the third stream (rb): ONE launch with a workgroup per level -- each waits inside the kernel for its level's sizes and
    // releases its level's fit (level 1's does not queue behind level 0's).  The merged order of the
    // correspondence kernels follows, beside the fits, and the read-back follows it in stream order.  (With events: a launch per level.)
    int size_classes_by_level() {
        SizeClassRange range[2];
        for (int l = 0; l < 2; ++l) {
            range[l] = SizeClassRange{1 << l, order_level[l], d_serial + 1 + l, DevSync()};
            if (sizes_dep[l]->by_counter()) {
                sizes_dep[l]->kernel_wait(range[l].sy);
                range[l].sy.signal_counter = classes_dep[l]->kernel_signal(p.rb, p.st[l]);
            } else {
                CHK(sizes_dep[l]->wait(p.rb, p.st[l]));
                launch_size_classes(nullptr, counts, &range[l], 1, p.rb, p.small_threshold, ctx->dbg.long_log2, gsize[0], gsize[1]);
                CHK(classes_dep[l]->signal(p.rb, p.st[l]));
            }
        }
        if (ctx->sizes0.by_counter()) launch_size_classes(nullptr, counts, range, 2, p.rb, p.small_threshold, ctx->dbg.long_log2, gsize[0], gsize[1]);
        return DMSA_OK;
    }
    // the read-back of the counts, the lattice tables and the device loop's previous result on the third stream, and the event sync #2 waits for
    int readback_copies() {
        if (ctx->dbg.one_readback != 0) {
            // lattice tables (incl. out_of_range), counts and the device loop's previous IterResult lie in one block in the host struct's layout: one
            // copy, 4-6 us, where three took 15 us in front of the host's one wait of the iteration
            HIPCHK(hipMemcpyAsync(ctx->rb(), ctx->d_readback.p, dmsa_ctx::kReadbackBytes, hipMemcpyDeviceToHost, p.rb));
        } else {
            HIPCHK(hipMemcpyAsync(&ctx->rb()->g, ctx->d_counts.p, sizeof(GaussCounts) + (p.by_level ? 3 : 1) * sizeof(SerialCounts), hipMemcpyDeviceToHost, p.rb));
            HIPCHK(hipMemcpyAsync(ctx->h_lattice, ctx->d_lattice.p, 2 * sizeof(LatticeTable), hipMemcpyDeviceToHost, p.rb));  // incl. out_of_range
            if (ctx->rb_extra_bytes)  // device loop: the previous iteration's stop decision travels with the counts
                HIPCHK(hipMemcpyAsync(ctx->rb_extra_dst, ctx->rb_extra_src, ctx->rb_extra_bytes, hipMemcpyDeviceToHost, p.rb));
        }
        HIPCHK(hipEventRecord(ctx->ev_counts, p.rb));
        return DMSA_OK;
    }
    int readback_common() {  // behind k_size_classes of the main stream
        if (!ctx->classes.by_counter()) CHK(ctx->classes.signal(ctx->stream, p.rb));  // (with counters k_size_classes gave the signal)
        CHK(ctx->classes.wait(p.rb, ctx->stream));
        return readback_copies();
    }
    // By level the read-back is enqueued BEHIND the fits: the host reaches their launches earlier, and the third stream has the classes of the
    // levels to run first anyway.  In front of it, beside the fits: the merged order of the correspondence kernels.
    int readback_by_level() {
        launch_size_classes(nullptr, counts, ctx->d_order.as<uint32_t>(), d_serial, p.rb, DevSync(), p.small_threshold, ctx->dbg.long_log2, 3, gsize[0], gsize[1]);
        return readback_copies();
    }

    // ---- the fit ----
    static int grow(int v) { return v + v / 8 + 16; }
    // one launch for the three size classes (and the rebalancing weights): no fork to a second stream, no join.  level < 0: the merged order.
    void launch_fit_classes(int level, const int first[3], const int tasks_in[3], bool weights, hipStream_t fs) {
        const int tasks[3] = {(ctx->dbg.fit_classes & 1) ? tasks_in[0] : 0, (ctx->dbg.fit_classes & 2) ? tasks_in[1] : 0, (ctx->dbg.fit_classes & 4) ? tasks_in[2] : 0};
        launch_gauss_fit_all(ctx->d_memb_local.as<float4>(), ctx->d_seg_off.as<int32_t>(), fit_table, level < 0 ? ctx->d_order.as<uint32_t>() : order_level[level],
                             reinterpret_cast<const int32_t*>(level < 0 ? d_serial : d_serial + 1 + level), first, tasks, ctx->d_fit_sums.as<float>(), counts,
                             ctx->d_info12.as<float>(), weights, ctx->rows - 1, ctx->d_gauss_rows.as<int2>(), ctx->dbg.eigen_l1_bytes, ctx->d_pow_codes.as<uint32_t>(),
                             (int)std::min<int64_t>(ctx->pow_n, INT32_MAX), ctx->d_memb_q.as<float>(), (size_t)(2 * ctx->n + 16), fs, p.by_level ? gsize[0] : nullptr,
                             gsize[1]);
    }
    int launch_finish(int finish_gauss) {
        launch_gauss_fit_finish(ctx->d_seg_off.as<int32_t>(), counts, ctx->d_fit_sums.as<float>(), finish_gauss, ctx->d_info12.as<float>(), ctx->stream);
        HIPCHK(hipGetLastError());
        return DMSA_OK;
    }
    // The speculated fit is enqueued BEHIND the read-back, with the previous iteration's class
    // counts (+ margin) as grids -- the kernels take the true ranges from device memory, surplus workgroups exit, and whatever the
    // guess missed is launched after sync #2 (rest_of_fit).
    int speculated_fit_common() {
        if (!ctx->vox.fit_guess_valid) return DMSA_OK;
        ScopedTimer tm(ctx, T_FIT);
        const int first0[3] = {0, 0, 0};
        const SerialCounts& pg = ctx->serial_counts;  // previous iteration
        fit_launched[2][0] = grow(pg.n_long), fit_launched[2][1] = grow(pg.n_chain - pg.n_long), fit_launched[2][2] = grow(pg.n_small);
        finish_launched = grow(pg.n_chain + pg.n_small);
        launch_fit_classes(-1, first0, fit_launched[2], true, ctx->stream), weights_launched = true;
        CHK(launch_finish(finish_launched));
        if (ctx->stamp_fit) launch_stamp(ctx->stamp_fit, ctx->stream);
        return DMSA_OK;
    }
    // By level: level l's fit follows its gather on its stream once its classes are there -- a one-wave wait that usually finds them (they ran
    // beside the gather).  Not a wait inside the fit: its 1024-thread workgroups take a compute unit's whole register file each, and a chip full
    // of them spinning would keep out whatever the third stream still has in front of the classes (the pose tables of a keyframe batch with a
    // thousand evaluations) until the waits give up (dev_sync.h, rule 2).  Level 1's launch is the one that runs when every size is known, so it
    // carries the weights.  Concurrent launches share no scratch: d_fit_sums and gauss_rows are indexed by Gaussian, d_memb_q by member offset,
    // everything else is LDS.
    // The main stream joins behind level 1's fit, launches the finish kernel and, last, the read-back (readback_by_level).
    int speculated_fit_and_readback_by_level() {
        ScopedTimer tm(ctx, T_FIT);
        const int first0[3] = {0, 0, 0};
        const bool guess = ctx->vox.fit_guess_valid && ctx->vox.fit_guess_level;
        for (int l = 0; l < 2 && guess; ++l) {
            const SerialCounts& pg = ctx->vox.serial_counts_level[l];
            fit_launched[l][0] = grow(pg.n_long), fit_launched[l][1] = grow(pg.n_chain - pg.n_long), fit_launched[l][2] = grow(pg.n_small);
            CHK(classes_dep[l]->wait(p.st[l], p.rb));
            launch_fit_classes(l, first0, fit_launched[l], l == 1, p.st[l]);
        }
        weights_launched = guess;
        // the main stream goes on behind level 1's gather (and fit); the same wave picks up the pose tables of the Jacobian batch, built on the side stream long ago
        WaitCarry also;
        ctx->tables.kernel_wait_owed(also.second_wait);
        CHK(ctx->fit1.signal(p.st[1], ctx->stream));
        CHK(ctx->fit1.wait(ctx->stream, p.st[1], 0, &also));
        if (guess) {
            finish_launched = grow(ctx->serial_counts.n_chain + ctx->serial_counts.n_small);
            CHK(launch_finish(finish_launched));
            if (ctx->stamp_fit) launch_stamp(ctx->stamp_fit, ctx->stream);
        }
        CHK(readback_by_level());
        HIPCHK(hipGetLastError());
        return DMSA_OK;
    }

    // ---- the two launch sequences, from the keys to the read-back ----
    // Common order: keys, sorts and leaves per level on the level's stream, both gathers and the size classes on the main stream, the read-back
    // on the third stream behind the classes, the speculated fit on the main stream behind them.  The one-launch path replaces everything up to the gathers.
    int common_order() {
        if (p.small) {
            CHK(small_path());
        } else {
            ScopedTimer tm(ctx, T_VOXEL);
            CHK(keys_and_sorts());
            CHK(leaves_of_both());
            CHK(gathers_common());
        }
        size_classes_common();
        if (ctx->stamp_voxel) launch_stamp(ctx->stamp_voxel, ctx->stream);
        CHK(readback_common());
        return speculated_fit_common();
    }
    // By level: keys, sorts, leaves AND gather per level on the level's stream, the classes of both levels on the third stream, each level's
    // fit on its stream behind its classes, then the main stream's join, the finish kernel and the read-back.
    int by_level_order() {
        {
            ScopedTimer tm(ctx, T_VOXEL);
            CHK(keys_and_sorts());
            CHK(leaves_of_both());
            CHK(gathers_by_level());
        }
        CHK(size_classes_by_level());
        if (ctx->stamp_voxel) launch_stamp(ctx->stamp_voxel, ctx->stream);
        return speculated_fit_and_readback_by_level();
    }

    // ---- sync #2 and what the host does behind it ----
    int wait_for_counts() {  // sync #2: M sizes every later launch
        hipError_t e;
        while ((e = hipEventQuery(ctx->ev_counts)) == hipErrorNotReady) {
        }
        (void)hipGetLastError();  // see sync_spin
        HIPCHK(e);
        return DMSA_OK;
    }
    int print_small_stamps() {  // debug switch gap_stamps = 3
        long long stamps[32];
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipMemcpy(stamps, ctx->d_sv_stamps.p, sizeof(stamps), hipMemcpyDeviceToHost));
        static int printed = 0;
        if (printed++ % 16 == 8) {
            for (int l = 0; l < 2; ++l) {
                std::fprintf(stderr, "[k_voxel_small level %d] us since its start:", l);
                for (int k = 1; k < 12; ++k) std::fprintf(stderr, " %.1f", (double)(stamps[l * 16 + k] - stamps[l * 16]) / 100.0);
                std::fprintf(stderr, "   (level start offset %.1f us)\n", (double)(stamps[l * 16] - stamps[0]) / 100.0);
            }
        }
        return DMSA_OK;
    }
    // The one redo: this build's speculation did not hold, so the voxelisation runs again, synchronously (no speculation: sync #1 brings the widths;
    // the caller's overlap and side_head work already ran).  Per reason:
    //
    //   reason          counters moved                              the re-run may        keying state afterwards
    //   SmallGaveUp     small_voxel_fallbacks                       not take the small    left alone (*)
    //                                                               path again
    //   TablesMoved     speculation_retries, keys_ahead_redone      as this build         cleared: the next build runs in the common order
    //   KeyLeftRange    speculation_retries                         not compress          cleared
    //   SortTooNarrow   speculation_retries                         as this build         cleared
    //
    // (*) looks accidental: the re-run takes the general path and may leave a keying set behind (hand_over_tables) that the other rows would
    //     withdraw.  Without effect today: the build that fell back was small, small implies !ahead_possible, and the next build of the same
    //     cloud is small again -- it does not go ahead and clears keying_valid itself.  Kept as it was.
    // In every case the width guesses are withdrawn first (VoxelState::redo), so that the re-run cannot speculate even where it may.
    int redo(Redo why) {
        BuildRequest again;
        again.allow_speculation = false, again.allow_compression = rq.allow_compression, again.allow_small = rq.allow_small;
        bool forget_keying = true;
        switch (why) {
            case Redo::SmallGaveUp:  // codes wider than 32 bits: the general path sorts them out
                ctx->small_voxel_fallbacks += 1;
                again.allow_small = false, forget_keying = false;
                break;
            case Redo::TablesMoved:  // the new table's range is right, only the guess was stale: compression stays allowed
                ctx->speculation_retries += 1, ctx->keys_ahead_redone += 1;
                break;
            case Redo::KeyLeftRange:  // a key left the predicted range: redo with full-width codes
                ctx->speculation_retries += 1;
                again.allow_compression = false;
                break;
            case Redo::SortTooNarrow:  // mis-speculated depth or width
                ctx->speculation_retries += 1;
                break;
        }
        return ctx->vox.redo(forget_keying, [&]() { return build_gaussians(ctx, s, again); });
    }
    // The verdict on the three speculations, behind sync #2: did the small path finish, were the tables the keys were made from the tables of this
    // cloud, did every key stay in the compressed range and below the guessed width?  *redone: the build was run again and the result is the re-run's.
    int verdict(bool* redone) {
        VoxelState& v = ctx->vox;
        *redone = false;
        h = ctx->rb()->g;
        if (p.small && ctx->dbg.gap_stamps == 3 && ctx->d_sv_stamps.p) CHK(print_small_stamps());
        if (p.small && (h.pad[0] != 0 || h.pad[1] != 0)) {  // codes wider than 32 bits (or a lattice error): the general path sorts them out
            if (ctx->h_lattice[0].status != 0) return ctx->h_lattice[0].status;
            if (ctx->h_lattice[1].status != 0) return ctx->h_lattice[1].status;
            return *redone = true, redo(Redo::SmallGaveUp);
        }
        if (p.ahead) {  // were the tables the keys were made from the tables of this cloud?
            bool stands = h.pad[2] == 0;  // (no key left the compressed range)
            for (int l = 0; l < 2; ++l) stands = stands && (!p.lvl_on[l] || same_keying_table(ctx->h_lattice[l], v.h_keying[l]));
            if (!stands) return *redone = true, redo(Redo::TablesMoved);
            for (int l = 0; l < 2; ++l)  // the level tags are the key kernel's, which wrote them to the keying set (dmsa_get_voxel_level reads the host's copy)
                ctx->h_lattice[l].code_or = v.h_keying[l].code_or = l == 0 ? 0ull : (1ull << p.tag_bit);
        }
        for (int l = 0; l < 2; ++l) {
            if (p.lvl_on[l] && ctx->h_lattice[l].status != 0) return ctx->h_lattice[l].status;
            const int true_bits = p.compress ? ctx->h_lattice[l].total_bits : 3 * ctx->h_lattice[l].final_depth;
            if (p.lvl_on[l] && p.compress && ctx->h_lattice[l].out_of_range) return *redone = true, redo(Redo::KeyLeftRange);
            if (!p.small && p.speculate && p.lvl_on[l] && (ctx->h_lattice[l].final_depth > p.sort_depth[l] || true_bits > p.sort_bits[l]))
                return *redone = true, redo(Redo::SortTooNarrow);
            if (p.lvl_on[l]) (ctx->h_lattice[l].pad3 ? ctx->lattice_hints_held : ctx->lattice_replays) += 1;
#ifdef DMSA_LATTICE_TIMING
            if (ctx->dbg.host_timeline != 0 && p.lvl_on[l]) {
                std::fprintf(stderr, "[k_lattice level %d hint %d] x10ns:", l, ctx->h_lattice[l].pad3);
                for (int k = 0; k < 8; ++k) std::fprintf(stderr, " %.0f", ctx->h_lattice[l].mn[kMaxLatticeEvents - 8 + k][0]);
                std::fprintf(stderr, "\n");
            }
#endif
            v.depth_guess[l] = ctx->h_lattice[l].final_depth;
            v.bits_guess[l] = ctx->h_lattice[l].total_bits;
            if (ctx->dbg.voxel_coherence != 0 && p.lvl_on[l]) {  // a different lattice re-labels every leaf: such a voxelisation could not reuse the previous order
                const LatticeTable &a = ctx->h_lattice[l], &b = ctx->coh_lattice[l];
                const bool same = a.final_depth == b.final_depth && a.compressed == b.compressed && std::memcmp(a.final_mn, b.final_mn, sizeof(a.final_mn)) == 0 &&
                                  std::memcmp(a.nbits, b.nbits, sizeof(a.nbits)) == 0 && std::memcmp(a.key_base, b.key_base, sizeof(a.key_base)) == 0;
                if (ctx->coh_pending[l] && !same) ctx->coh_lattice_changes += 1;
                ctx->coh_lattice[l] = a, ctx->coh_pending[l] = false;
            }
        }
        return DMSA_OK;
    }
    // whatever the pre-sync launches did not cover (first iteration, or a class that grew by more than the margin), and the sizes of the result
    int rest_of_fit() {
        VoxelState& v = ctx->vox;
        {
            ScopedTimer tm(ctx, T_FIT);
            const int M_all = h.level[0].num_gauss + h.level[1].num_gauss;
            ctx->serial_counts = ctx->rb()->sc;
            const SerialCounts& sc = ctx->serial_counts;
            // (by level: per level on the main stream, which is behind both gathers; the weights with level 1's unless they ran already)
            int any = 0;
            for (int k = p.by_level ? 0 : 2; k < (p.by_level ? 2 : 3) && M_all > 0; ++k) {
                const SerialCounts& lc = k == 2 ? sc : (v.serial_counts_level[k] = ctx->rb()->sc_level[k]);
                const int want[3] = {lc.n_long, lc.n_chain - lc.n_long, lc.n_small};
                int rest[3], some = 0;
                for (int c = 0; c < 3; ++c) rest[c] = std::max(0, want[c] - fit_launched[k][c]), some += rest[c];
                const bool weights = k == 2 ? some > 0 || finish_launched < M_all : (k == 1 && !weights_launched);
                if (some > 0 || weights) launch_fit_classes(k == 2 ? -1 : k, fit_launched[k], rest, weights, ctx->stream);
                any += some;
            }
            if (M_all > 0 && (any > 0 || finish_launched < M_all)) CHK(launch_finish(M_all));
            v.fit_guess_level = p.by_level && M_all > 0;
            v.fit_guess_valid = M_all > 0;
            ctx->order_valid = true;
        }
        HIPCHK(hipGetLastError());
        ctx->M1 = h.level[0].num_gauss;
        ctx->M = h.level[0].num_gauss + h.level[1].num_gauss;
        ctx->Mm = (int64_t)h.level[0].num_memb + h.level[1].num_memb;
        ctx->gaussians_valid = true;
        return DMSA_OK;
    }
    // the hand-over of this build's tables to the next build's keying set, and the streak that lets the next build go ahead
    int hand_over_tables() {
        VoxelState& v = ctx->vox;
        if (p.ahead) {
            for (int l = 0; l < 2; ++l) ctx->keys_ahead_held += p.lvl_on[l] ? 1 : 0;
            v.keying_streak += 1;
        } else if (p.ahead_possible) {
            // this cloud's tables become the keying set of the next voxelisation: every kernel that wrote them is through (the host has read them), and
            // the next reader follows the main stream's next transform.  (Only behind a voxelisation in the common order: the first one behind an
            // upload, and the one behind a redo.)
            bool same = v.keying_host_valid && v.keying_n == p.n;
            for (int l = 0; l < 2; ++l) same = same && (!p.lvl_on[l] || same_keying_table(ctx->h_lattice[l], v.h_keying[l]));
            v.keying_streak = same ? v.keying_streak + 1 : 0;
            v.h_keying[0] = ctx->h_lattice[0], v.h_keying[1] = ctx->h_lattice[1];
            v.keying_host_valid = true, v.keying_n = p.n;
            v.keying_valid = ctx->dbg.keys_ahead >= 2 || v.keying_streak >= kKeysAheadStreak;  // the rule of keys_ahead = 1 (kKeysAheadStreak)
            if (v.keying_valid)
                HIPCHK(hipMemcpyAsync(ctx->d_keying.p, ctx->d_lattice.p, 2 * sizeof(LatticeTable), hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            v.keying_valid = false, v.keying_host_valid = false;
        }
        return DMSA_OK;
    }
};

}  // namespace

// ---- Gaussians (DmsaOptimizer.h:78-96) ---------------------------------------------------------------------
int build_gaussians(dmsa_ctx* ctx, const dmsa_settings& s, const BuildRequest& rq) {
    VoxelState& v = ctx->vox;
    ctx->gaussians_valid = false;
    ctx->order_valid = false;
    ctx->M = 0, ctx->M1 = 0, ctx->Mm = 0;
    ctx->voxel_calls += 1;
    if (rq.allow_speculation && ctx->dbg.speculation_fault > 0 && ctx->voxel_calls == ctx->dbg.speculation_fault)  // test hook: a guess one level too shallow
        for (int l = 0; l < 2; ++l) {
            if (v.depth_guess[l] > 1) v.depth_guess[l] -= 1;
            if (v.bits_guess[l] > 3) v.bits_guess[l] -= 3;
        }
    VoxelPlan plan = make_plan(ctx, s, rq);
    // createGaussianSets(set, factor * minGridSize, ...): float product, widened to double by the octree constructor
    ctx->level_res[0] = (double)(s.grid_size_1_factor * ctx->min_grid_size);
    ctx->level_res[1] = (double)(s.grid_size_2_factor * ctx->min_grid_size);
    if (!plan.lvl_on[0]) ctx->level_res[0] = ctx->level_res[1];
    if (!plan.lvl_on[1]) ctx->level_res[1] = ctx->level_res[0];
    VoxelBuild b(ctx, s, rq, plan);

    if (!plan.ahead && rq.side_head) CHK(rq.side_head());  // (ahead: behind k_lattice on the third stream, lattice_aside)
    CHK(b.lattice_main());                    // not speculating: ends with sync #1 ...
    CHK(resolve_sort_widths(ctx, plan));      // ... whose depths complete the plan
    CHK(b.split_scratch());
    CHK(plan.by_level ? b.by_level_order() : b.common_order());  // keys, sorts, leaves, gathers, size classes, read-back, speculated fit
    ctx->tl.mark("voxel enq");
    if (rq.overlap) CHK(rq.overlap());
    ctx->tl.mark("jacobian batch host+enq");
    CHK(b.wait_for_counts());                 // sync #2
    ctx->tl.mark("sync#2 wait");
    bool redone = false;
    const int rc = b.verdict(&redone);        // a speculation that did not hold: the build has run again (VoxelBuild::redo)
    if (redone || rc != DMSA_OK) return rc;
    CHK(b.rest_of_fit());
    return b.hand_over_tables();
}
