// voxelize_driver.cpp — currentGauss.reset() + createGaussianSets at both resolutions + Gaussian fit + updateRebalancingWeights
// (DmsaOptimizer.h:78-96) as one launch sequence over three streams; kernels in dmsa_kernels.hip / radix_sort.hip / serial_kernels.hip.
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

// ---- Gaussians (DmsaOptimizer.h:78-96) ---------------------------------------------------------------------
// `overlap` (optional) runs on the host after every voxelisation kernel has been enqueued and before the counts are read
// back: host work placed there hides behind the GPU.
int build_gaussians(dmsa_ctx* ctx, const dmsa_settings& s, const std::function<int()>& overlap, bool allow_speculation, bool allow_compression, bool allow_small,
                    const std::function<int()>& side_head) {
    const int64_t n = ctx->n;
    ctx->gaussians_valid = false;
    ctx->order_valid = false;
    ctx->M = 0, ctx->M1 = 0, ctx->Mm = 0;
    const bool lvl_on[2] = {s.grid_size_1_factor > std::numeric_limits<float>::min(), s.grid_size_2_factor > std::numeric_limits<float>::min()};
    // createGaussianSets(set, factor * minGridSize, ...): float product, widened to double by the octree constructor
    ctx->level_res[0] = (double)(s.grid_size_1_factor * ctx->min_grid_size);
    ctx->level_res[1] = (double)(s.grid_size_2_factor * ctx->min_grid_size);
    if (!lvl_on[0]) ctx->level_res[0] = ctx->level_res[1];
    if (!lvl_on[1]) ctx->level_res[1] = ctx->level_res[0];
    const bool compress = ctx->dbg.key_compress != 0 && allow_compression;
    // The reference's everyday size (5 scans x <= 3000 points + static points): ONE launch from the lattice to the member lists, a workgroup per
    // resolution (small_voxel.hip).  The kernel takes the tree depths and code widths from the lattice table on the device: nothing to
    // speculate on, no second stream, no joins.  Codes wider than 32 bits make it give up (counts.pad) and the general path runs.
    const bool small = allow_small && ctx->dbg.small_voxel != 0 && n <= small_voxel_max_points() && lvl_on[0] && lvl_on[1] &&
                       !(s.gauss_split != 0 && ctx->model == MODEL_KEYFRAMES) && ctx->dbg.voxel_coherence == 0;
    ctx->voxel_calls += 1;
    if (allow_speculation && ctx->dbg.speculation_fault > 0 && ctx->voxel_calls == ctx->dbg.speculation_fault)  // test hook: a guess one level too shallow
        for (int l = 0; l < 2; ++l) {
            if (ctx->depth_guess[l] > 1) ctx->depth_guess[l] -= 1;
            if (ctx->bits_guess[l] > 3) ctx->bits_guess[l] -= 3;
        }
    const bool speculate = small || (allow_speculation && ctx->depth_guess[0] >= 0 && ctx->depth_guess[1] >= 0 && ctx->depth_guess[0] < 20 && ctx->depth_guess[1] < 20 &&
                                     (!compress || (ctx->bits_guess[0] >= 0 && ctx->bits_guess[1] >= 0)));
    // the key kernels count the digits of the sort that follows (own sort, 32-bit codes): no clearing kernel, no histogram pass
    const bool prehist = ctx->dbg.sort_prehist != 0;
    // The two resolutions are independent until their member lists are appended (level 1 starts at level 0's totals):
    // level 0 runs on `stream`, level 1 on `stream2`; their launches are enqueued stage by stage so that both streams fill.
    const bool two = ctx->dbg.dual_stream != 0 && lvl_on[0] && lvl_on[1];
    hipStream_t st[2] = {ctx->stream, two ? ctx->stream2 : ctx->stream};
    // Each level's size classes, gather and fit behind its own leaf scan (debug switch fit_by_level; see the launch sequence below).  The sizes come
    // from k_leaf_finalize, so the single-workgroup scan and the one-launch path keep the common order.
    // 1 (default) goes by size, like small_threshold: windows of a few ten thousand points are bound by the host's launches, and this order has more of
    // them (the 25 360-point IMU window: 3686-3817 against 4027-4063 it/s); 2: whatever the size.  The 200 000 is a guess between the measured points,
    // not a measured crossover: slower at 25 360 points, 1-3 % faster at the 140 000-point rosette window (which the rule leaves out), at the
    // keyframe pass and at 1.5 M points.
    const bool by_level = (ctx->dbg.fit_by_level >= 2 || (ctx->dbg.fit_by_level == 1 && n >= 200000)) && two && !small && ctx->dbg.fused_leaf_scan != 0;
    int32_t* const gsize[2] = {ctx->d_gauss_size[0].as<int32_t>(), ctx->d_gauss_size[1].as<int32_t>()};
    uint32_t* lattice_signal = nullptr;  // k_lattice carries the signal for level 1's stream (dev_sync.h), one per resolution
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
    // Rule of keys_ahead = 1: only behind kKeysAheadStreak consecutive voxelisations of the context whose tables did not change (the host compares
    // each read-back set with the one before; an upload and a redo start the count again).  A redo costs a whole voxelisation (~250 us on the
    // bench window) where the ahead order saves ~21 us, so it pays below one redo in about twelve builds; the first iterations on a new cloud
    // are far above that (the 140 000-point rosette window: 5 redos in its first 25 iterations, none in the 180 behind them, and 20-step runs
    // 3 % below the parent with the rule "wherever possible"), the converged ones far below.  8 is a guess between those, not a measured optimum.
    // The device copy of the set is made only when the next build may use it.
    constexpr int kKeysAheadStreak = 8;
    // (also left to the common order: one stream for everything, and stage timers, whose event pairs would bracket other streams' kernels)
    const bool ahead_possible = ctx->dbg.keys_ahead != 0 && ctx->dbg.dual_stream != 0 && ctx->dbg.lattice_hint != 0 && !prehist && !small && n > 0 &&
                                (ctx->flags & DMSA_FLAG_STAGE_TIMERS) == 0;
    bool ahead = false;
    if (ahead_possible && speculate && ctx->lattice_hint_valid && ctx->keying_valid && ctx->keying_n == n) {
        // Codes of either width: the width follows the guess in both orders, and a sort of 64-bit codes clears its own header.  (The window of
        // the bench has 32-bit codes; the near-miss clouds of the tests, whose far outlier makes a box of depth 13, have 38-bit ones.)
        ahead = true;
        for (int l = 0; l < 2; ++l) ahead = ahead && ctx->h_keying[l].compressed == (compress ? 1 : 0);
    }
    LatticeTable* const key_tab = ahead ? ctx->d_keying.as<LatticeTable>() : ctx->d_lattice.as<LatticeTable>();
    if (!ahead && side_head) CHK(side_head());
    {
        ScopedTimer tm(ctx, T_VOXEL);
        const int nb = (int)((n + kAabbBlock - 1) / kAabbBlock);
        if (!ctx->aabb_fresh)  // the device loop's fused transform already left the block bounds and cleared the counters
            launch_block_aabb(ctx->d_global.as<float4>(), n, ctx->d_aabb.as<float>(), ctx->d_counts.p, sizeof(GaussCounts) + sizeof(SerialCounts),
                              ctx->stream);
        ctx->aabb_fresh = false;
        // the lattice kernel clears the headers of the own radix sorts on the side (one dispatch less per sort)
        if (!small && !ahead) lattice_signal = ctx->lattice.kernel_signal(ctx->stream, st[1], 2);
        if (!ahead)  // (ahead: on the third stream, behind the first key kernel's launch -- below)
            launch_lattice(ctx->d_global.as<float4>(), n, ctx->d_aabb.as<float>(), nb, ctx->level_res[0], ctx->level_res[1], compress,
                           ctx->d_lattice.as<LatticeTable>(), ctx->d_sort_tmp[0].p, ctx->d_sort_tmp[1].p, ctx->stream,
                           lattice_signal, ctx->dbg.lattice_hint != 0 && ctx->lattice_hint_valid);
        ctx->lattice_hint_valid = true;  // (a table of another problem is harmless: it fails the verification and the replay runs)
        if (!speculate) {  // sync #1: tree depths select the radix-sort bit range (speculation reads them with the counts instead)
            HIPCHK(hipMemcpyAsync(ctx->h_lattice, ctx->d_lattice.p, 2 * sizeof(LatticeTable), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(sync_spin(ctx->stream));
        }
    }
    // The sort only needs an UPPER bound of the tree depth.  From the second iteration on the previous depths are used
    // without waiting for the lattice kernel; the true depths arrive with the counts (sync #2) and a too-small guess (the
    // bounding box doubled between two iterations) re-runs the voxelisation synchronously.
    int sort_depth[2], sort_bits[2];
    for (int l = 0; l < 2; ++l) {
        sort_depth[l] = speculate ? ctx->depth_guess[l] : ctx->h_lattice[l].final_depth;
        // width of the leaf codes: all 3*depth bits, or (compressed) only the bits that vary over the points
        sort_bits[l] = !compress ? 3 * sort_depth[l] : (speculate ? ctx->bits_guess[l] : ctx->h_lattice[l].total_bits);
        if (!speculate && lvl_on[l] && ctx->h_lattice[l].status != 0) return ctx->h_lattice[l].status;
    }
    GaussCounts* counts = ctx->d_counts.as<GaussCounts>();
    const bool split = s.gauss_split != 0 && ctx->model == MODEL_KEYFRAMES;
    if (split && !ctx->d_split_stats.p) {
        HIPCHK(ctx->d_split_stats.ensure(64 * 16));  // 64 stripes of (blocks looked at, blocks skipped)
        HIPCHK(hipMemsetAsync(ctx->d_split_stats.p, 0, 64 * 16, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));  // (both level streams add to it)
    }
    if (split)
        for (int l = 0; l < 2; ++l) {
            HIPCHK(ctx->d_pos_slot_rank[l].ensure((size_t)n * 4));
            HIPCHK(ctx->d_nsorted[l].ensure((size_t)n * 16));
            HIPCHK(ctx->d_pair_d[l].ensure(split_scratch_bytes(n)));
        }
    bool k32v[2] = {false, false};
    // Both resolutions are keyed into one array of 2n (code, point) pairs -- level 1 carries a tag bit above the widest code --
    // and sorted by ONE radix sort: half the launches, twice the parallelism per pass, and the sorted halves are the two levels.
    if (ctx->dbg.trace_time >= 3) std::fprintf(stderr, "[voxelize] key bits (without the marker of non-finite points): level 0 %d, level 1 %d\n", sort_bits[0], sort_bits[1]);
    const int tag_bit = std::max(sort_bits[0], sort_bits[1]) + 1;  // bit `sort_bits` is the marker of non-finite points
    const unsigned end_bit = (unsigned)(tag_bit + 1);
    const bool k32 = small || end_bit <= 32;  // (the small path writes 32-bit codes or gives up)
    {
        const size_t ksz = k32 ? 4 : 8;
        for (int l = 0; l < 2; ++l) {
            k32v[l] = ctx->key32[l] = k32;
            ctx->code_v[l] = ctx->d_code[0].as<char>() + (size_t)l * n * ksz, ctx->code_s_v[l] = ctx->d_code_s[0].as<char>() + (size_t)l * n * ksz;
            ctx->idx_v[l] = ctx->d_idx[0].as<uint32_t>() + (size_t)l * n, ctx->idx_s_v[l] = ctx->d_idx_s[0].as<uint32_t>() + (size_t)l * n;
        }
    }
    // Small clouds (keyframe sets: 3 x 10^5 points) are launch-bound: one sort of 2n pairs on one stream.  Large clouds (the window:
    // 1.5 x 10^6) keep the two levels on two streams with one sort each (a sort only looks at the bits below its end bit, so the
    // tag is inert there).
    const bool merged = ctx->dbg.merge_sort < 0 ? n <= (int64_t)(1 << 20) : ctx->dbg.merge_sort != 0;
    const bool prepared = prehist && k32;
    const int items = ctx->dbg.sort_items;  // the plans below and the sorts they describe are given the same tile choice
    SortPlan plan[2];  // merged: one sort of 2n pairs in workspace 0, both key kernels count into its header
    for (int l = 0; l < 2 && !small; ++l)
        plan[l] = merged ? sort_pairs_u32_plan(ctx->d_sort_tmp[0].p, (size_t)(2 * n), end_bit, items)
                         : sort_pairs_u32_plan(ctx->d_sort_tmp[l].p, (size_t)n, (unsigned)(sort_bits[l] + 1), items);
    uint32_t* ahead_signal = nullptr;  // ahead: "the transform is through", given by the first key kernel of the main stream as it starts
    auto stage_keys = [&](int l, hipStream_t stream) {  // a disabled level is keyed with the other level's lattice (level_res is aliased) and ignored later
        SortPlan pl = plan[l];
        if (merged && l == 1) pl.state_words = 0;  // the look-back words of the common sort are cleared once
        VoxelKeysAhead ka;
        if (ahead) {
            ka.range_flag = &counts->pad[2];
            if (k32 && !(merged && l == 1)) ka.clear_header = reinterpret_cast<uint32_t*>(plan[l].header);
            if (stream == ctx->stream) ka.start_signal = ahead_signal, ahead_signal = nullptr;
        }
        launch_voxel_keys(ctx->d_global.as<float4>(), n, key_tab + l, ctx->level_res[l], ctx->code_v[l], k32, ctx->idx_v[l],
                          l == 0 ? 0ull : (1ull << tag_bit), prepared ? &pl : nullptr, stream, ka);
        if (ctx->dbg.voxel_coherence != 0 && lvl_on[l]) {  // how many points changed leaf since the previous voxelisation of this context
            const size_t ksz = k32 ? 4 : 8;
            const bool compare = ctx->coh_valid[l] && ctx->d_code_prev[l].cap >= (size_t)n * ksz && ctx->coh_key32[l] == k32 && ctx->coh_n[l] == n;
            if (ctx->d_code_prev[l].ensure((size_t)n * ksz) != hipSuccess || ctx->d_coh_count.ensure(8) != hipSuccess) return;
            if (!ctx->coh_count_zeroed) (void)hipMemsetAsync(ctx->d_coh_count.p, 0, 8, stream), ctx->coh_count_zeroed = true;
            launch_count_code_changes(ctx->code_v[l], ctx->d_code_prev[l].p, k32, n, compare, ctx->d_coh_count.as<unsigned long long>(), stream);
            if (compare) ctx->coh_compared += n;
            ctx->coh_pending[l] = compare;
            ctx->coh_valid[l] = true, ctx->coh_key32[l] = k32, ctx->coh_n[l] = n;
        }
    };
    auto stage_sort_both = [&]() -> int {
        stage_keys(0, ctx->stream), stage_keys(1, ctx->stream);
        if (k32 && prepared)
            HIPCHK(sort_pairs_u32_onesweep(ctx->d_sort_tmp[0].p, ctx->d_sort_tmp[0].cap, ctx->d_code[0].as<uint32_t>(), ctx->d_code_s[0].as<uint32_t>(),
                                           ctx->d_idx[0].as<uint32_t>(), ctx->d_idx_s[0].as<uint32_t>(), (size_t)(2 * n), end_bit, items, ctx->stream, 2));
        else if (k32)
            HIPCHK(sort_pairs_u32_u32(ctx->d_sort_tmp[0].p, ctx->d_sort_tmp[0].cap, ctx->d_code[0].as<uint32_t>(), ctx->d_code_s[0].as<uint32_t>(),
                                      ctx->d_idx[0].as<uint32_t>(), ctx->d_idx_s[0].as<uint32_t>(), (size_t)(2 * n), end_bit, items, ctx->stream, true /* the lattice kernel cleared the header */));
        else
            HIPCHK(sort_pairs_u64_u32(ctx->d_sort_tmp[0].p, ctx->d_sort_tmp[0].cap, ctx->d_code[0].as<uint64_t>(), ctx->d_code_s[0].as<uint64_t>(),
                                      ctx->d_idx[0].as<uint32_t>(), ctx->d_idx_s[0].as<uint32_t>(), (size_t)(2 * n), end_bit, items, ctx->stream));
        return DMSA_OK;
    };
    auto stage_sort = [&](int l) -> int {
        stage_keys(l, st[l]);
        const unsigned eb = (unsigned)(sort_bits[l] + 1);
        if (k32 && prepared)
            HIPCHK(sort_pairs_u32_onesweep(ctx->d_sort_tmp[l].p, ctx->d_sort_tmp[l].cap, (const uint32_t*)ctx->code_v[l], (uint32_t*)ctx->code_s_v[l], ctx->idx_v[l],
                                           ctx->idx_s_v[l], (size_t)n, eb, items, st[l], 2));
        else if (k32)
            HIPCHK(sort_pairs_u32_u32(ctx->d_sort_tmp[l].p, ctx->d_sort_tmp[l].cap, (const uint32_t*)ctx->code_v[l], (uint32_t*)ctx->code_s_v[l], ctx->idx_v[l],
                                      ctx->idx_s_v[l], (size_t)n, eb, items, st[l], true /* the lattice kernel cleared the header */));
        else
            HIPCHK(sort_pairs_u64_u32(ctx->d_sort_tmp[l].p, ctx->d_sort_tmp[l].cap, (const uint64_t*)ctx->code_v[l], (uint64_t*)ctx->code_s_v[l], ctx->idx_v[l],
                                      ctx->idx_s_v[l], (size_t)n, eb, items, st[l]));
        return DMSA_OK;
    };
    auto stage_leaves = [&](int l) -> int {
        const LatticeTable* tab = key_tab + l;
        const bool k32 = k32v[l];
        if (ctx->dbg.fused_segments != 0) {
            // one single-pass kernel; its look-back state is never cleared (epoch-tagged words, running ticket counter)
            ChainedScanCall call;
            HIPCHK(ctx->seg_state[l].begin((size_t)leaf_segment_tiles(n), kLeafSegmentWords, st[l], &call));
            launch_leaf_segments(ctx->code_s_v[l], k32, n, tab, ctx->d_leaf_incl[l].as<int32_t>(), ctx->d_leaf_start[l].as<int32_t>(), &counts->level[l], call, st[l]);
        } else {
            launch_head_flags(ctx->code_s_v[l], k32, n, tab, ctx->d_head[l].as<int32_t>(), st[l]);
            HIPCHK(inclusive_scan_i32(ctx->d_scan_tmp[l].p, ctx->d_scan_tmp[l].cap, ctx->d_head[l].as<int32_t>(), ctx->d_leaf_incl[l].as<int32_t>(), (size_t)n, st[l]));
            launch_leaf_starts(ctx->d_head[l].as<int32_t>(), ctx->d_leaf_incl[l].as<int32_t>(), ctx->code_s_v[l], k32, tab, n,
                               ctx->d_leaf_start[l].as<int32_t>(), &counts->level[l], st[l]);
        }
        launch_leaf_accept(ctx->d_leaf_start[l].as<int32_t>(), ctx->idx_s_v[l], ctx->d_ring.as<int32_t>(), &counts->level[l],
                           s.min_num_points_per_set, n, ctx->d_slot_acc[l].as<int32_t>(), ctx->d_slot_cnt[l].as<int32_t>(), st[l]);
        if (split)
            launch_leaf_split(ctx->d_leaf_incl[l].as<int32_t>(), ctx->d_leaf_start[l].as<int32_t>(), ctx->idx_s_v[l], ctx->d_ring.as<int32_t>(),
                              ctx->d_nglobal.as<float4>(), &counts->level[l], s.min_num_points_per_set, n, ctx->d_nsorted[l].as<float4>(),
                              ctx->d_pair_d[l].as<unsigned long long>(), ctx->d_slot_acc[l].as<int32_t>(), ctx->d_slot_cnt[l].as<int32_t>(),
                              ctx->d_pos_slot_rank[l].as<int32_t>(), st[l], ctx->dbg.skip_stats != 0 ? ctx->d_split_stats.as<unsigned long long>() : nullptr);
        // slot scans: one multi-workgroup single-pass kernel (debug switch fused_leaf_scan = 0: the single-workgroup k_leaf_scan)
        if (ctx->dbg.fused_leaf_scan != 0) {
            ChainedScanCall call;
            HIPCHK(ctx->fin_state[l].begin((size_t)leaf_finalize_tiles(n), kLeafFinalizeWords, st[l], &call));
            launch_leaf_finalize(ctx->d_slot_acc[l].as<int32_t>(), ctx->d_slot_cnt[l].as<int32_t>(), n, ctx->d_gauss_of_slot[l].as<int32_t>(),
                                 ctx->d_memb_of_slot[l].as<int32_t>(), &counts->level[l], call, st[l], by_level ? gsize[l] : nullptr);
        } else
            launch_leaf_scan(ctx->d_slot_acc[l].as<int32_t>(), ctx->d_slot_cnt[l].as<int32_t>(), ctx->d_gauss_of_slot[l].as<int32_t>(), ctx->d_memb_of_slot[l].as<int32_t>(),
                             &counts->level[l], st[l]);
        return DMSA_OK;
    };
    auto stage_gather = [&](int l, hipStream_t gs, uint32_t* start_signal = nullptr) {
        const LatticeTable* tab = key_tab + l;
        launch_gather_members(ctx->d_leaf_incl[l].as<int32_t>(), ctx->d_leaf_start[l].as<int32_t>(), ctx->idx_s_v[l],
                              ctx->code_s_v[l], k32v[l], tab, ctx->d_slot_acc[l].as<int32_t>(), ctx->d_gauss_of_slot[l].as<int32_t>(),
                              ctx->d_memb_of_slot[l].as<int32_t>(), split ? ctx->d_pos_slot_rank[l].as<int32_t>() : nullptr, ctx->d_local.as<float4>(),
                              ctx->d_slot_cnt[l].as<int32_t>(), counts, l, n, ctx->d_memb_local.as<float4>(), ctx->d_memb_idx.as<int32_t>(),
                              ctx->d_memb_g.as<int32_t>(), ctx->d_seg_off.as<int32_t>(), gs, start_signal);
    };
    if (small) {
        ScopedTimer tm(ctx, T_VOXEL);
        SmallVoxelArgs a{};
        a.global = ctx->d_global.as<float4>(), a.local = ctx->d_local.as<float4>(), a.ring = ctx->d_ring.as<int32_t>();
        a.n = (int)n, a.min_pts = s.min_num_points_per_set;
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
    } else {
        ScopedTimer tm(ctx, T_VOXEL);
        // k_lattice of the ahead order: on the third stream, as soon as the transform is through, in front of whatever the caller has for that stream
        auto lattice_aside = [&]() -> int {
            CHK(ctx->lattice.wait(ctx->stream3, ctx->stream));
            launch_lattice(ctx->d_global.as<float4>(), n, ctx->d_aabb.as<float>(), (int)((n + kAabbBlock - 1) / kAabbBlock), ctx->level_res[0], ctx->level_res[1],
                           compress, ctx->d_lattice.as<LatticeTable>(), nullptr, nullptr, ctx->stream3, nullptr, true, key_tab);
            if (side_head) CHK(side_head());
            return DMSA_OK;
        };
        if (ahead) {
            // The first key kernel of the main stream says, as it starts, that the transform is through (events: recorded in front of it); the waits
            // of the other two streams are enqueued behind the main stream's own kernels -- a wait enqueued ahead of them has its queue served
            // first and they start late (the measured rule below).
            ahead_signal = ctx->lattice.kernel_signal(ctx->stream, ctx->stream3);
            if (!ahead_signal) CHK(ctx->lattice.signal(ctx->stream, ctx->stream3));
        }
        if (merged) CHK(stage_sort_both());
        if (ahead && merged) CHK(lattice_aside());  // (before the signal behind the common sort is counted: this wait is for the key kernel's alone)
        // level 1 on its own stream: it needs the lattice (k_lattice signalled; ahead: the transform) and, merged, the common sort (a signal behind it;
        // with events the one signal)
        if (merged || (!ahead && !lattice_signal)) CHK(ctx->lattice.signal(ctx->stream, st[1]));
        if (!merged && ahead) {
            bool waited = false;  // the main stream's level first: its key kernel carries the signal
            for (int l = 0; l < 2; ++l)
                if (lvl_on[l] && st[l] == ctx->stream) CHK(stage_sort(l));
            for (int l = 0; l < 2; ++l)
                if (lvl_on[l] && st[l] != ctx->stream) {
                    if (!waited) CHK(ctx->lattice.wait(st[l], ctx->stream));
                    waited = true;
                    CHK(stage_sort(l));
                }
            CHK(lattice_aside());
        } else {
            CHK(ctx->lattice.wait(st[1], ctx->stream));
            if (!merged)
                for (int l = 0; l < 2; ++l)
                    if (lvl_on[l]) CHK(stage_sort(l));
        }
        // (Enqueueing level 1 first -- its chain ends last -- was measured in round 5: 1089 instead of 1259 it/s.  Level 1's first kernel sits behind
        // a device-side wait; launched ahead of level 0's kernels the wait's queue is served first and level 0 starts late.
        // Swapping the streams as well -- level 1 on the main stream and enqueued first, level 0 behind the wait on the side stream -- was also
        // measured: 1243 against 1263 it/s on the headline window, the small windows and the keyframe set unchanged.)
        for (int l = 0; l < 2; ++l) {
            if (!lvl_on[l]) continue;
            CHK(stage_leaves(l));
        }        // Both gathers on the first stream (level 1 appends behind level 0's totals anyway): the level-1 chain ends with its leaf scan,
        // long before level 0's gather is through, so the wait below finds its event signalled -- a join at the END of a stream costs
        // ~20 us of cross-queue signalling in front of everything that follows.
        if (!by_level) {
            CHK(ctx->level1.signal(st[1], ctx->stream));
            if (lvl_on[0]) stage_gather(0, ctx->stream);
            CHK(ctx->level1.wait(ctx->stream, st[1]));
            if (lvl_on[1]) stage_gather(1, ctx->stream);
        } else {
            // By level: the kernel behind a level's k_leaf_finalize says that the sizes and totals of the level are final (its size classes on the
            // third stream may run) -- level 0's gather as it starts; on level 1's stream the one-wave wait for level 0's totals, behind which
            // level 1's members are appended (they are known long before: the wait finds them there), once it is through: level 1's Gaussians are
            // numbered behind level 0's, so its signal stands for both levels.
            uint32_t* sig = ctx->sizes0.kernel_signal(st[0], ctx->stream3);
            if (!sig) CHK(ctx->sizes0.signal(st[0], ctx->stream3));
            stage_gather(0, st[0], sig);
            WaitCarry carry;
            carry.pass_on = ctx->sizes1.kernel_signal(st[1], ctx->stream3);
            CHK(ctx->sizes0.wait(st[1], st[0], 0, &carry));
            if (!carry.pass_on) CHK(ctx->sizes1.signal(st[1], ctx->stream3));  // (events: recorded behind the wait)
            stage_gather(1, st[1]);
        }
    }
    // The read-back of the counts runs on the third stream: a device-to-host copy ends with a system-scope release that holds up the
    // stream it is on for ~20 us, and the fit behind it does not need to wait for that.
    hipStream_t rb = ctx->dbg.dual_stream != 0 ? ctx->stream3 : ctx->stream;
    // Which Gaussians walk their members on one lane group (k_residuals_small, the fit's one-wave class) and which get a workgroup
    // (chain tiers, the fit's four-wave class)?  The lane-per-evaluation kernel spends the fewest instructions per member, but a wave of
    // it walks up to `threshold` members one after the other: with a few thousand Gaussians (the reference's everyday windows, small
    // keyframe sets) its few hundred waves leave the chip idle while the longest of them runs.  Measured (it/s at thresholds 8 = nobody /
    // 32 / 256, scripts/threshold_ab.sh): config-2 window, 1100 Gaussians 3450 / 3090 / 2580; 8 keyframes, 2465: 1965 / 1955 / 1906;
    // 12 keyframes, 3823: 1672 / 1782 / 1726; 16 keyframes, 4920: 1353 / 1534 / 1502; 24 keyframes, 6906: 910 / 1080 / 1213; the bench
    // window, 13 000: - / 1196 (64) / 1262.  Every tier computes the same bits, so the rule may follow the size of the previous
    // voxelisation (the first one of a context goes by the number of points).
    const int auto_threshold = ctx->M > 0 ? (ctx->M < 2000 ? 8 : ctx->M < 6000 ? 32 : 0) : (n < 60000 ? 8 : n < 200000 ? 32 : 0);
    const int small_threshold = ctx->dbg.small_threshold > 0 ? ctx->dbg.small_threshold : auto_threshold;
    SerialCounts* const d_serial = reinterpret_cast<SerialCounts*>(ctx->d_counts.as<char>() + sizeof(GaussCounts));  // merged | level 0 | level 1
    uint32_t* const order_level[2] = {ctx->d_order_level.as<uint32_t>(), ctx->d_order_level.as<uint32_t>() + n + 8};
    StreamDep* const sizes_dep[2] = {&ctx->sizes0, &ctx->sizes1};
    StreamDep* const classes_dep[2] = {&ctx->classes0, &ctx->classes1};
    if (!by_level) {   // size classes of the correspondence kernels: needs only seg_off, so it runs before the read-back
        // k_size_classes is one workgroup on the main stream between the voxelisation and the fit: it also carries two stream dependencies
        // (dev_sync.h) -- it waits for the pose tables of the Jacobian batch (built on the side stream long ago) and releases the read-back
        DevSync sy;
        ctx->tables.kernel_wait_owed(sy);
        sy.signal_counter = ctx->classes.kernel_signal(ctx->stream, rb);
        launch_size_classes(ctx->d_seg_off.as<int32_t>(), counts, ctx->d_order.as<uint32_t>(), d_serial, ctx->stream, sy, small_threshold, ctx->dbg.long_log2);
    } else {
        // By level, all on the third stream (rb): ONE launch with a workgroup per level -- each waits inside the kernel for its level's sizes and
        // releases its level's fit (level 1's does not queue behind level 0's).  The merged order of the
        // correspondence kernels follows, beside the fits, and the read-back follows it in stream order.  (With events: a launch per level.)
        SizeClassRange range[2];
        for (int l = 0; l < 2; ++l) {
            range[l] = SizeClassRange{1 << l, order_level[l], d_serial + 1 + l, DevSync()};
            if (sizes_dep[l]->by_counter()) {
                sizes_dep[l]->kernel_wait(range[l].sy);
                range[l].sy.signal_counter = classes_dep[l]->kernel_signal(rb, st[l]);
            } else {
                CHK(sizes_dep[l]->wait(rb, st[l]));
                launch_size_classes(nullptr, counts, &range[l], 1, rb, small_threshold, ctx->dbg.long_log2, gsize[0], gsize[1]);
                CHK(classes_dep[l]->signal(rb, st[l]));
            }
        }
        if (ctx->sizes0.by_counter()) launch_size_classes(nullptr, counts, range, 2, rb, small_threshold, ctx->dbg.long_log2, gsize[0], gsize[1]);
    }
    if (ctx->stamp_voxel) launch_stamp(ctx->stamp_voxel, ctx->stream);
    // the read-back of the counts on the third stream; by level it is enqueued BEHIND the fits (below): the host reaches their launches earlier,
    // and the third stream has the classes of the levels to run first anyway
    auto enqueue_readback = [&]() -> int {
        if (!by_level) {
            if (!ctx->classes.by_counter()) CHK(ctx->classes.signal(ctx->stream, rb));  // (with counters k_size_classes gave the signal)
            CHK(ctx->classes.wait(rb, ctx->stream));
        } else {  // the merged order of the correspondence kernels, beside the fits
            launch_size_classes(nullptr, counts, ctx->d_order.as<uint32_t>(), d_serial, rb, DevSync(), small_threshold, ctx->dbg.long_log2, 3, gsize[0], gsize[1]);
        }
        if (ctx->dbg.one_readback != 0) {
            // lattice tables (incl. out_of_range), counts and the device loop's previous IterResult lie in one block in the host struct's layout: one
            // copy, 4-6 us, where three took 15 us in front of the host's one wait of the iteration
            HIPCHK(hipMemcpyAsync(ctx->rb(), ctx->d_readback.p, dmsa_ctx::kReadbackBytes, hipMemcpyDeviceToHost, rb));
        } else {
            HIPCHK(hipMemcpyAsync(&ctx->rb()->g, ctx->d_counts.p, sizeof(GaussCounts) + (by_level ? 3 : 1) * sizeof(SerialCounts), hipMemcpyDeviceToHost, rb));
            HIPCHK(hipMemcpyAsync(ctx->h_lattice, ctx->d_lattice.p, 2 * sizeof(LatticeTable), hipMemcpyDeviceToHost, rb));  // incl. out_of_range
            if (ctx->rb_extra_bytes)  // device loop: the previous iteration's stop decision travels with the counts
                HIPCHK(hipMemcpyAsync(ctx->rb_extra_dst, ctx->rb_extra_src, ctx->rb_extra_bytes, hipMemcpyDeviceToHost, rb));
        }
        HIPCHK(hipEventRecord(ctx->ev_counts, rb));
        return DMSA_OK;
    };
    if (!by_level) CHK(enqueue_readback());
    // The fit is enqueued BEHIND the read-back, with the previous iteration's class
    // counts (+ margin) as grids -- the kernels take the true ranges from device memory, surplus workgroups exit, and whatever the
    // guess missed is launched after sync #2.  The three classes run side by side on two streams (each is latency-bound on its own).
    const float* fit_table = ctx->base_table ? ctx->base_table : ctx->d_tables.as<float>();
    // one launch for the three size classes (and the rebalancing weights): no fork to a second stream, no join.  level < 0: the merged order.
    auto launch_fit_classes = [&](int level, const int first[3], const int tasks_in[3], bool weights, hipStream_t fs) {
        const int tasks[3] = {(ctx->dbg.fit_classes & 1) ? tasks_in[0] : 0, (ctx->dbg.fit_classes & 2) ? tasks_in[1] : 0, (ctx->dbg.fit_classes & 4) ? tasks_in[2] : 0};
        launch_gauss_fit_all(ctx->d_memb_local.as<float4>(), ctx->d_seg_off.as<int32_t>(), fit_table, level < 0 ? ctx->d_order.as<uint32_t>() : order_level[level],
                             reinterpret_cast<const int32_t*>(level < 0 ? d_serial : d_serial + 1 + level), first, tasks, ctx->d_fit_sums.as<float>(), counts,
                             ctx->d_info12.as<float>(), weights, ctx->rows - 1, ctx->d_gauss_rows.as<int2>(), ctx->dbg.eigen_l1_bytes, ctx->d_pow_codes.as<uint32_t>(),
                             (int)std::min<int64_t>(ctx->pow_n, INT32_MAX), ctx->d_memb_q.as<float>(), (size_t)(2 * ctx->n + 16), fs, by_level ? gsize[0] : nullptr,
                             gsize[1]);
    };
    auto launch_finish = [&](int finish_gauss) -> int {
        launch_gauss_fit_finish(ctx->d_seg_off.as<int32_t>(), counts, ctx->d_fit_sums.as<float>(), finish_gauss, ctx->d_info12.as<float>(), ctx->stream);
        HIPCHK(hipGetLastError());
        return DMSA_OK;
    };
    int fit_launched[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}} /* [level; 2 = merged][class] */, finish_launched = 0;
    bool weights_launched = false;
    const int first0[3] = {0, 0, 0};
    auto grow = [](int v) { return v + v / 8 + 16; };
    if (!by_level) {
        if (ctx->fit_guess_valid) {
            ScopedTimer tm(ctx, T_FIT);
            const SerialCounts& pg = ctx->serial_counts;  // previous iteration
            fit_launched[2][0] = grow(pg.n_long), fit_launched[2][1] = grow(pg.n_chain - pg.n_long), fit_launched[2][2] = grow(pg.n_small);
            finish_launched = grow(pg.n_chain + pg.n_small);
            launch_fit_classes(-1, first0, fit_launched[2], true, ctx->stream), weights_launched = true;
            CHK(launch_finish(finish_launched));
            if (ctx->stamp_fit) launch_stamp(ctx->stamp_fit, ctx->stream);
        }
    } else {
        // By level: level l's fit follows its gather on its stream once its classes are there -- a one-wave wait that usually finds them (they ran
        // beside the gather).  Not a wait inside the fit: its 1024-thread workgroups take a compute unit's whole register file each, and a chip full
        // of them spinning would keep out whatever the third stream still has in front of the classes (the pose tables of a keyframe batch with a
        // thousand evaluations) until the waits give up (dev_sync.h, rule 2).  Level 1's launch is the one that runs when every size is known, so it
        // carries the weights.  Concurrent launches share no scratch: d_fit_sums and gauss_rows are indexed by Gaussian, d_memb_q by member offset,
        // everything else is LDS.
        ScopedTimer tm(ctx, T_FIT);
        const bool guess = ctx->fit_guess_valid && ctx->fit_guess_level;
        for (int l = 0; l < 2 && guess; ++l) {
            const SerialCounts& pg = ctx->serial_counts_level[l];
            fit_launched[l][0] = grow(pg.n_long), fit_launched[l][1] = grow(pg.n_chain - pg.n_long), fit_launched[l][2] = grow(pg.n_small);
            CHK(classes_dep[l]->wait(st[l], rb));
            launch_fit_classes(l, first0, fit_launched[l], l == 1, st[l]);
        }
        weights_launched = guess;
        // the main stream goes on behind level 1's gather (and fit); the same wave picks up the pose tables of the Jacobian batch, built on the side stream long ago
        WaitCarry also;
        ctx->tables.kernel_wait_owed(also.second_wait);
        CHK(ctx->fit1.signal(st[1], ctx->stream));
        CHK(ctx->fit1.wait(ctx->stream, st[1], 0, &also));
        if (guess) {
            finish_launched = grow(ctx->serial_counts.n_chain + ctx->serial_counts.n_small);
            CHK(launch_finish(finish_launched));
            if (ctx->stamp_fit) launch_stamp(ctx->stamp_fit, ctx->stream);
        }
        CHK(enqueue_readback());
        HIPCHK(hipGetLastError());
    }
    ctx->tl.mark("voxel enq");
    if (overlap) CHK(overlap());
    ctx->tl.mark("jacobian batch host+enq");
    {  // sync #2: M sizes every later launch
        hipError_t e;
        while ((e = hipEventQuery(ctx->ev_counts)) == hipErrorNotReady) {
        }
        (void)hipGetLastError();  // see sync_spin
        HIPCHK(e);
    }
    ctx->tl.mark("sync#2 wait");
    const GaussCounts h = ctx->rb()->g;
    if (small && ctx->dbg.gap_stamps == 3 && ctx->d_sv_stamps.p) {
        long long st[32];
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipMemcpy(st, ctx->d_sv_stamps.p, sizeof(st), hipMemcpyDeviceToHost));
        static int printed = 0;
        if (printed++ % 16 == 8) {
            for (int l = 0; l < 2; ++l) {
                std::fprintf(stderr, "[k_voxel_small level %d] us since its start:", l);
                for (int k = 1; k < 12; ++k) std::fprintf(stderr, " %.1f", (double)(st[l * 16 + k] - st[l * 16]) / 100.0);
                std::fprintf(stderr, "   (level start offset %.1f us)\n", (double)(st[l * 16] - st[0]) / 100.0);
            }
        }
    }
    if (small && (h.pad[0] != 0 || h.pad[1] != 0)) {  // codes wider than 32 bits (or a lattice error): the general path sorts them out
        if (ctx->h_lattice[0].status != 0) return ctx->h_lattice[0].status;
        if (ctx->h_lattice[1].status != 0) return ctx->h_lattice[1].status;
        ctx->small_voxel_fallbacks += 1;
        ctx->depth_guess[0] = ctx->depth_guess[1] = -1;
        return build_gaussians(ctx, s, nullptr, false, allow_compression, false);
    }
    if (ahead) {  // the verdict: were the tables the keys were made from the tables of this cloud?
        bool stands = h.pad[2] == 0;  // (no key left the compressed range)
        for (int l = 0; l < 2; ++l) stands = stands && (!lvl_on[l] || same_keying_table(ctx->h_lattice[l], ctx->h_keying[l]));
        if (!stands) {  // redo in the common order; the new table's range is right, only the guess was stale: compression stays allowed
            ctx->depth_guess[0] = ctx->depth_guess[1] = -1;
            ctx->speculation_retries += 1, ctx->keys_ahead_redone += 1;
            const int rc = build_gaussians(ctx, s, nullptr, false, allow_compression, allow_small);
            ctx->keying_valid = false, ctx->keying_streak = 0;
            return rc;
        }
        for (int l = 0; l < 2; ++l)  // the level tags are the key kernel's, which wrote them to the keying set (dmsa_get_voxel_level reads the host's copy)
            ctx->h_lattice[l].code_or = ctx->h_keying[l].code_or = l == 0 ? 0ull : (1ull << tag_bit);
    }
    for (int l = 0; l < 2; ++l) {
        if (lvl_on[l] && ctx->h_lattice[l].status != 0) return ctx->h_lattice[l].status;
        const int true_bits = compress ? ctx->h_lattice[l].total_bits : 3 * ctx->h_lattice[l].final_depth;
        if (lvl_on[l] && compress && ctx->h_lattice[l].out_of_range) {
            ctx->depth_guess[0] = ctx->depth_guess[1] = -1;
            ctx->speculation_retries += 1;
            const int rc = build_gaussians(ctx, s, nullptr, false, false, allow_small);  // a key left the predicted range: redo with full-width codes
            ctx->keying_valid = false, ctx->keying_streak = 0;
            return rc;
        }
        if (!small && speculate && lvl_on[l] && (ctx->h_lattice[l].final_depth > sort_depth[l] || true_bits > sort_bits[l])) {
            ctx->depth_guess[0] = ctx->depth_guess[1] = -1;
            ctx->speculation_retries += 1;
            const int rc = build_gaussians(ctx, s, nullptr, false, allow_compression, allow_small);  // mis-speculated: redo (overlap work already ran)
            ctx->keying_valid = false, ctx->keying_streak = 0;
            return rc;
        }
        if (lvl_on[l]) (ctx->h_lattice[l].pad3 ? ctx->lattice_hints_held : ctx->lattice_replays) += 1;
#ifdef DMSA_LATTICE_TIMING
        if (ctx->dbg.host_timeline != 0 && lvl_on[l]) {
            std::fprintf(stderr, "[k_lattice level %d hint %d] x10ns:", l, ctx->h_lattice[l].pad3);
            for (int k = 0; k < 8; ++k) std::fprintf(stderr, " %.0f", ctx->h_lattice[l].mn[kMaxLatticeEvents - 8 + k][0]);
            std::fprintf(stderr, "\n");
        }
#endif
        ctx->depth_guess[l] = ctx->h_lattice[l].final_depth;
        ctx->bits_guess[l] = ctx->h_lattice[l].total_bits;
        if (ctx->dbg.voxel_coherence != 0 && lvl_on[l]) {  // a different lattice re-labels every leaf: such a voxelisation could not reuse the previous order
            const LatticeTable &a = ctx->h_lattice[l], &b = ctx->coh_lattice[l];
            const bool same = a.final_depth == b.final_depth && a.compressed == b.compressed && std::memcmp(a.final_mn, b.final_mn, sizeof(a.final_mn)) == 0 &&
                              std::memcmp(a.nbits, b.nbits, sizeof(a.nbits)) == 0 && std::memcmp(a.key_base, b.key_base, sizeof(a.key_base)) == 0;
            if (ctx->coh_pending[l] && !same) ctx->coh_lattice_changes += 1;
            ctx->coh_lattice[l] = a, ctx->coh_pending[l] = false;
        }
    }
    {
        ScopedTimer tm(ctx, T_FIT);
        const int M_all = h.level[0].num_gauss + h.level[1].num_gauss;
        // whatever the pre-sync launches did not cover (first iteration, or a class that grew by more than the margin)
        ctx->serial_counts = ctx->rb()->sc;
        const SerialCounts& sc = ctx->serial_counts;
        // (by level: per level on the main stream, which is behind both gathers; the weights with level 1's unless they ran already)
        int any = 0;
        for (int k = by_level ? 0 : 2; k < (by_level ? 2 : 3) && M_all > 0; ++k) {
            const SerialCounts& lc = k == 2 ? sc : (ctx->serial_counts_level[k] = ctx->rb()->sc_level[k]);
            const int want[3] = {lc.n_long, lc.n_chain - lc.n_long, lc.n_small};
            int rest[3], some = 0;
            for (int c = 0; c < 3; ++c) rest[c] = std::max(0, want[c] - fit_launched[k][c]), some += rest[c];
            const bool weights = k == 2 ? some > 0 || finish_launched < M_all : (k == 1 && !weights_launched);
            if (some > 0 || weights) launch_fit_classes(k == 2 ? -1 : k, fit_launched[k], rest, weights, ctx->stream);
            any += some;
        }
        if (M_all > 0 && (any > 0 || finish_launched < M_all)) CHK(launch_finish(M_all));
        ctx->fit_guess_level = by_level && M_all > 0;
        ctx->fit_guess_valid = M_all > 0;
        ctx->order_valid = true;
    }
    HIPCHK(hipGetLastError());
    ctx->M1 = h.level[0].num_gauss;
    ctx->M = h.level[0].num_gauss + h.level[1].num_gauss;
    ctx->Mm = (int64_t)h.level[0].num_memb + h.level[1].num_memb;
    ctx->gaussians_valid = true;
    if (ahead) {
        for (int l = 0; l < 2; ++l) ctx->keys_ahead_held += lvl_on[l] ? 1 : 0;
        ctx->keying_streak += 1;
    } else if (ahead_possible) {
        // this cloud's tables become the keying set of the next voxelisation: every kernel that wrote them is through (the host has read them), and
        // the next reader follows the main stream's next transform.  (Only behind a voxelisation in the common order: the first one behind an
        // upload, and the one behind a redo.)
        bool same = ctx->keying_host_valid && ctx->keying_n == n;
        for (int l = 0; l < 2; ++l) same = same && (!lvl_on[l] || same_keying_table(ctx->h_lattice[l], ctx->h_keying[l]));
        ctx->keying_streak = same ? ctx->keying_streak + 1 : 0;
        ctx->h_keying[0] = ctx->h_lattice[0], ctx->h_keying[1] = ctx->h_lattice[1];
        ctx->keying_host_valid = true, ctx->keying_n = n;
        ctx->keying_valid = ctx->dbg.keys_ahead >= 2 || ctx->keying_streak >= kKeysAheadStreak;
        if (ctx->keying_valid)
            HIPCHK(hipMemcpyAsync(ctx->d_keying.p, ctx->d_lattice.p, 2 * sizeof(LatticeTable), hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        ctx->keying_valid = false, ctx->keying_host_valid = false;
    }
    return DMSA_OK;
}

