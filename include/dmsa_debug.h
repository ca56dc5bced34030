/*
 * dmsa_debug.h — debug / experiment switches of a dmsa_ctx.
 *
 * Production code never needs this header: dmsa_create() (dmsa_hip.h) uses the defaults listed here.  The switches select between
 * implementations that produce THE SAME RESULTS (tests run both sides of each); they exist for A/B timing, for bisecting, and for the
 * parity tests that exercise a fallback on purpose.  tests/test_gpu_size_edges.py runs serial_streams, sort_prehist, overlap_batch,
 * stream_priority, long_log2, sort_items (every tile size, one child process each), small_threshold, long_split, serial_tree, shared_rotations,
 * eval_skip, small_voxel, device_loop and eigen_l1_bytes on a cloud with one Gaussian per member count around every size boundary of the kernels;
 * the other switches: tests/test_gpu_loop.py, tests/test_gpu_configs.py, tests/test_gpu_large_keyframe_sets.py, tests/test_gpu_small_voxel.py,
 * tests/test_gpu_fit_by_level.py, tests/test_gpu_batch_timer.py.
 * They are fixed when the context is created:
 *
 *   dmsa_create_ex2(device, flags, &options, sizeof options, &ctx)   from code, or
 *   DMSA_DEBUG="name=value,name=value" in the environment: read ONCE by dmsa_create / dmsa_create_ex / dmsa_create_ex2, overrides fields
 *                                                      by name (profiling scripts).  It is the only environment variable the library reads.
 *
 * Six switches have no field in the struct and are set by name, through dmsa_create_named or DMSA_DEBUG:
 *   batch_stamps   1   a residual batch whose tiers run on more than one stream (a latency tier exists, device_sync on) is timed by the device's
 *                      wall clock inside kernels it has anyway: the latency tier's first workgroup stores the clock, the join's wait kernel adds the
 *                      difference to a tick accumulator the call reads once at its end (dmsa_timing::residual_kernel_ms, include/dmsa_hip.h).  Every
 *                      other batch, and every batch with 0, is timed by a HIP-event pair on the main stream, whose two barrier packets idle that
 *                      stream for 6-7 us each.  Same bits (tests/test_gpu_batch_timer.py); bench window 1292 -> 1307 it/s
 *                      (profiles/r15_batch_stamps_ab.txt).
 *   one_readback   1   the host's one wait per iteration follows ONE device-to-host copy (lattice tables, counts, per-level size classes and the
 *                      device loop's previous IterResult lie in one block in the layout of the host's struct); 0: a copy each.  Inside the spread at
 *                      the bench size (same file).
 *   fit_by_level   1   general voxelisation path with both levels on two streams: each level's size classes, member gather and Gaussian fit follow
 *                      its own k_leaf_finalize (level 1 on the second stream, the size classes and the merged order of the correspondence kernels
 *                      on the third), instead of both gathers, one k_size_classes and one fit in series on the main stream (0).  1: from 200 000
 *                      points on (smaller windows are bound by the host's launches, of which this order has more: the 25 360-point IMU window is
 *                      6 % slower with it); 2: whatever the size.  Same bits (tests/test_gpu_fit_by_level.py); bench window 1260 -> 1289 it/s
 *                      (profiles/r11_fit_by_level_ab.txt).
 *   next_head      1   device loop, window model without IMU rows, from the second iteration of a call on: the base pose table is not computed by
 *                      k_window_pose_tables at the head of the iteration.  It is the table of the line-search trial that just won, which that batch
 *                      evaluated from the same control poses, or the previous base table when none won; the kernel that transforms the points reads
 *                      it through the index k_loop_finish leaves on the device and copies it to where the fit reads it.  0: computed as before;
 *                      1 and 2: on (no size rule was needed); 3: on, IMU windows included, and the table is also computed and compared word by word
 *                      (dmsa_debug_next_head).  Off by rule for IMU windows (every evaluation rewrites relative pose 0), keyframe sets and contexts
 *                      with stage timers.  Same bits (tests/test_gpu_next_head.py); measured in profiles/r18_next_head_ab.txt.
 *   ne_triangle    1   normal equations up to 64 parameters: k_normal_eq_source computes the block sums of the elements i <= j only (one workgroup
 *                      per row block and tile pair ti <= tj instead of four per tile, the operands fetched, formed and staged once, 2 x 2 outputs
 *                      per thread), and the consumer -- the LM step's loader in the device loop, k_normal_eq_reduce_upper elsewhere -- adds half as
 *                      many block sums and gives (j, i) the bits of (i, j).  0: k_normal_eq_partial and the full square as before.  Above 64
 *                      parameters nothing changes.  Same bits, NaN signs included (tests/test_gpu_ne_triangle.py); measured in
 *                      profiles/r20_ne_triangle_ab.txt.
 *   keys_ahead     1   general voxelisation path, speculated (from the second voxelisation behind an upload on): the key kernel and
 *                      the sort of each level follow the transform directly and read the lattice tables the PREVIOUS voxelisation ended with (a set
 *                      of its own that nothing writes meanwhile); k_lattice runs beside them on the third stream, verifies that set as its hint and
 *                      writes this cloud's tables, and at the iteration's one wait the host compares the two sets field by field.  Equal: the
 *                      voxelisation is the one the common order gives.  Different (a trigger met another box, the global bounds crossed a cell): it
 *                      is redone in the common order, counted as a speculation retry, and the build behind a redo runs in the common order too.
 *                      0: keys behind k_lattice; 2: wherever possible; 1: only behind eight consecutive voxelisations of the context whose tables did
 *                      not change -- the first iterations on a new cloud change them too often for a redo to pay (the rosette window: 5 redos in
 *                      its first 25 iterations, none in the next 180).  Not with sort_prehist, dual_stream = 0,
 *                      lattice_hint = 0 or stage timers.  Same bits (tests/test_gpu_keys_ahead.py); counters: dmsa_debug_keys_ahead.
 */
#ifndef DMSA_DEBUG_H
#define DMSA_DEBUG_H

#include "dmsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmsa_debug_options {
    int32_t device_loop;     /* 1   optimizeSet's control state lives on the device (csrc/loop_kernels.hip); 0: the host drives the loop
                                     (three waits per iteration, as in rounds 1-2)                                                        */
    int32_t dual_stream;     /* 1   the two voxel resolutions and the count read-back on their own streams; 0: everything on one stream   */
    int32_t serial_streams;  /* 3   streams the three tiers of the reference-order correspondence kernels run on (1, 2 or 3)              */
    int32_t merge_sort;      /* 0   one radix sort per voxel level, on two streams; 1: both levels in ONE sort of 2 n pairs (level 1 tagged above the
                                     widest code); -1: merged up to 2^20 points (the rule of rounds 2-4, from before the stream dependencies moved
                                     to device counters: round 5 measured separate sorts 1-2.5 % faster at every size, profiles/r05_ab_merge_sort.txt) */
    int32_t key_compress;    /* 1   drop the key bits that are equal for all points before sorting; 0: full 3 x depth bit leaf codes
                                     (64-bit codes, sorted as two 32-bit halves, from depth 11 on -- also the fallback of a mis-predicted range) */
    int32_t fused_segments;  /* 1   head flags + scan + leaf starts in one single-pass kernel; 0: three kernels (csrc/radix_sort.hip's scan)  */
    int32_t sort_prehist;    /* 0   the key kernels count the sort digits (measured 1.5 % slower than the sort's own histogram pass)     */
    int32_t overlap_batch;   /* 1   host-driven loop only: host math of the Jacobian batch while the GPU voxelises                        */
    int32_t serial_tree;     /* 1   double sum of the chain tiers: 1 parallel reduction when the exactness test allows it,
                                     0 always the member-order chain, 2 both and keep the chain's result (test hook).  Where the test fails
                                     for a Gaussian of the latency tier, only the BLOCKS of its member list whose own bounds fail are chained
                                     (csrc/serial_kernels.hip); 3 (test hook): every block through that chain                               */
    int32_t host_threads;    /* 16  worker threads of the context (upload packing, host-built pose tables, host solve)                   */
    int32_t solve_threads;   /* 12  of which the blocked host LM solve uses at most this many                                            */
    int32_t host_timeline;   /* 0   print host-side time stamps of the last iteration of every optimize call to stderr                   */
    int32_t trace_time;      /* 0   print upload / optimize wall time of dmsa_optimize_window to stderr                                  */
    int32_t fused_leaf_scan; /* 1   slot scans of the accepted leaves as a multi-workgroup single-pass kernel; 0: the                
                                     single-workgroup k_leaf_scan                                                                         */
    int32_t device_sync;     /* 1   fork / join of the three tier streams through counters in device memory (one-wave signal / wait
                                     kernels); 0: hipEventRecord / hipStreamWaitEvent                                                   */
    int32_t shared_rotations; /* 1  forward differences of translation parameters share the rotated member coordinates of evaluation 0 in
                                     the second pass of the chain tiers (serial_kernels.hip); 0: every evaluation transforms on its own     */
    int32_t eval_skip;       /* 1   a (Gaussian, evaluation) pair of the Jacobian batch whose pose-table rows all have evaluation 0's bits is not
                                     computed: its residual IS evaluation 0's (csrc/serial_kernels.hip); 0: every pair is computed;
                                     2: every pair is computed and the pairs 1 would have skipped are compared (dmsa_eval_skip_stats)       */
    int32_t sync_fault;      /* 0   test hook: k > 0 withholds the signal of the k-th device-side wait of every whole call -- the wait
                                     gives up, the library restores the state of the call's start and runs it again with events            */
    int32_t speculation_fault; /* 0 test hook: k > 0 plants a tree depth one too small in the k-th voxelisation of every whole call, so the
                                     speculative sort width is wrong and the voxelisation runs again                                       */
    int32_t voxel_coherence; /* 0   1: count, per voxelisation and level, the points whose leaf code differs from the previous voxelisation's of
                                     the same context (dmsa_debug_counters: how much of last iteration's sorted order would survive)       */
    int32_t lm_stream;       /* 1   LM solve for 64 < P <= 192 as a stream of pivot-step records (one wave per 8 columns, csrc/loop_kernels.hip:
                                     k_loop_lm_stream); 0: column-block workgroups handing panels over (k_loop_lm_panels).  Same bits.        */
    int32_t stream_priority; /* 0   bit 0 / 1 / 2: the main / second / third stream of the context is created at the device's highest priority
                                     (which of the concurrent kernels of an iteration the wave dispatcher serves first)                      */
    int32_t gap_stamps;      /* 0   1: one-thread kernels write the device's wall clock in front of, between and behind the kernels of the normal
                                     equations and the LM solve of every iteration; the gaps of the LAST iteration of a call are printed to stderr
                                     -- what the kernel trace of a profiler cannot tell: whether the holes it shows between those kernels
                                     exist when no profiler slows the host's launches.  2: also eight stamps per iteration (begin, voxelisation,
                                     fit, Jacobian batch, normal equations, LM step, trial chains + tables, end), printed as a table             */
    int32_t lattice_hint;    /* 1   k_lattice first checks, in parallel, whether the bounding-box growth events of the previous voxelisation of this
                                     context still hold for the moved points (same result as the replay, proved per launch); 0: always the
                                     sequential replay of PCL's adoptBoundingBoxToPoint                                                    */
    int32_t fit_classes;     /* 7   PROFILING ONLY (results are wrong unless 7): bit 0 / 1 / 2 = the Gaussian fit runs its long / middle / short
                                     size class -- how much of k_gauss_fit_all's time belongs to which class                              */
    int32_t eigen_l1_bytes;  /* 32768  NOT an A/B switch: the L1 data cache size of the machine the REFERENCE runs on.  Eigen sizes the depth
                                     blocks kc of centered^T * centered (Gaussians.h:147) from it at run time (32768 -> 680, 49152 -> 1016), and
                                     the float sum of a Gaussian with more members than kc depends on kc.  Set it to that machine's L1d to
                                     reproduce its bits; Gaussians up to kc members do not depend on it.                                  */
    int32_t small_threshold; /* 0   members up to which a Gaussian goes to the lane-per-evaluation correspondence kernel (and the fit's one-wave class);
                                     0 = the built-in rule (previous voxelisation: < 2000 Gaussians nobody, < 6000 up to 32 members, else 256), else 1 .. 256.
                                     Every tier computes the same bits.                                                                  */
    int32_t skip_stats;      /* 0   1: k_jacobian_columns counts, per evaluation, the (Gaussian, evaluation) pairs eval_skip left out and (eval_skip = 2)
                                     the ones that differed after all -> counters skip_pairs_equal / skip_mismatches; k_split_pairs counts the pair
                                     blocks it looked at and skipped -> split_blocks / split_blocks_skipped.  Off by default: atomics on the
                                     path of every iteration (two per wave and evaluation in k_jacobian_columns)                          */
    /* ---- appended in round 6; from here on the struct is APPEND-ONLY (no field is removed or moved) and dmsa_create_ex2 takes its size ---- */
    int32_t small_voxel;     /* 0   1: point sets of at most 32 768 points (the reference's everyday windows: 5 scans x <= 3000 points + static points) are
                                     voxelised by ONE launch -- a workgroup per resolution keeps its (code, point) pairs in registers from the leaf codes to
                                     the member lists (csrc/small_voxel.hip) -- instead of ten dependent kernels per level; 0 (default): always the general path.
                                     Same bits.                                                                                              */
    int32_t long_split;      /* 1   latency tier (Gaussians of >= 4096 members) of a window with at most 16 of them, B <= 32: the workgroup of a (Gaussian,
                                     sub-batch) ends with its float chain, leaves the means in device memory, and 8 HELPER workgroups per item -- blocks at the
                                     end of the same launch -- sum a slice of the members each (the parallel second pass; the last one to arrive tests the
                                     exactness bounds and runs the member-by-member chain itself if they fail).  >= 2: that many members as the threshold, in
                                     every batch of every model (experiments); 0: every workgroup does its own second pass.  Same bits.             */
    int32_t long_log2;       /* 0   Gaussians of at least 2^long_log2 members go to the latency tier of the correspondence kernels (10 waves per workgroup,
                                     helpers); 0 = the built-in rule (12), else 9 .. 20.  Every tier computes the same bits.                          */
    int32_t sort_items;      /* 0   EXPERIMENTS ONLY: pairs per thread of a tile of the onesweep sort (512 threads) in every sort of this context: 2, 4, 8 or
                                     16; 0 (or any other value) = by size (2 up to 2^16 pairs, 4 up to 2^18, else 16).  Same bits.            */
    int32_t trial_rows_aside; /* 1  window with IMU rows, device loop: the nine trial chains of the line search write their control poses on the main stream
                                     and compute their additional rows on the side stream, beside the trial batch (0: one kernel, in front of it).  Same bits. */
} dmsa_debug_options;

/* what the switches above leave behind, since the context was created */
typedef struct dmsa_debug_counters {
    int64_t sync_retries;         /* whole calls run again with event dependencies after a device-side wait gave up           */
    int64_t speculation_retries;  /* voxelisations run again because the speculated sort width was too small                  */
    int64_t skip_pairs;           /* (Gaussian, evaluation) pairs of the Jacobian batches the eval_skip logic looked at       */
    int64_t skip_pairs_equal;     /* ... of which had the pose-table rows of evaluation 0 (eval_skip = 1: were not computed) */
    int64_t skip_mismatches;      /* eval_skip = 2 only: such pairs whose computed residual differed from evaluation 0's      */
    int64_t split_blocks;         /* splitSet search (gauss_split): blocks of 64 positions x 64 partners looked at ...       */
    int64_t split_blocks_skipped; /* ... and skipped because their normals cannot be within 0.5 of anti-parallel       */
    int64_t voxel_codes_compared; /* voxel_coherence = 1: (point, level) pairs compared with the previous voxelisation            */
    int64_t voxel_codes_changed;  /* ... whose leaf code changed                                                               */
    int64_t lattice_hints_held;   /* lattice_hint: (voxelisation, level) pairs whose previous growth events were verified instead of replayed ... */
    int64_t lattice_replays;      /* ... and pairs that went through the sequential replay                                       */
    int64_t voxel_lattice_changes;/* ... voxelisations (per level) whose lattice (origin, depth, code bits) differed from the previous one's:
                                     every code of that level counts as changed                                                 */
    /* appended in round 6 (append-only like the options) */
    int64_t small_voxel_launches; /* small_voxel: voxelisations that went through the one-launch path (csrc/small_voxel.hip) ...        */
    int64_t small_voxel_fallbacks;/* ... and how many of them it handed back to the general path (leaf codes wider than 32 bits) */
} dmsa_debug_counters;
int dmsa_get_debug_counters(dmsa_ctx* ctx, dmsa_debug_counters* out);
/* What the switch next_head left behind since the context was created (the counter struct above is pinned field by field and does not grow for it):
 * out2[0] = iterations whose base table was adopted from the previous line search instead of computed, out2[1] = 32-bit words in which an adopted
 * table differed from the computed one (counted with next_head = 3 only; any value but 0 is a bug). */
int dmsa_debug_next_head(dmsa_ctx* ctx, int64_t* out2);
/* What the switch keys_ahead left behind since the context was created: out2[0] = (voxelisation, level) pairs whose keys were made ahead of
 * k_lattice, from the previous voxelisation's tables, and stood (counted like lattice_hints_held); out2[1] = voxelisations keyed ahead whose
 * tables turned out to differ and that were redone in the common order (each also counts as a speculation retry). */
int dmsa_debug_keys_ahead(dmsa_ctx* ctx, int64_t* out2);
/* Test hook (fit_by_level): the size classes the last voxelisation of the context sorted EACH level into -- out[4 l + 0 .. 3] = Gaussians of level l
 * in the fit's long / middle / short class and its largest Gaussian (members); out[8] = 1 if that voxelisation ran by level, else 0 (and zeros). */
int dmsa_debug_level_size_classes(dmsa_ctx* ctx, int32_t* out9);
/* Test hook: pow(-1) of `count` member counts as the Gaussian fit computes it on the device (Gaussians.h:172: libm's powf(n, -1.0f) through
 * the difference table of the host's libm; counts[] and out[] are host arrays; counts above 2^24 are refused). */
int dmsa_debug_pow_minus_one(dmsa_ctx* ctx, const int32_t* counts, int32_t count, float* out);
/* Test hook: Gaussians::limitCovariance (Gaussians.h:181-201) as the fit computes it on the device, on `count` column-major 3 x 3 matrices (host arrays):
 * out9 = V max(D, 1e-4) V^-1; optionally the EigenSolver<Matrix3f> behind it -- eigenvalues().real() in the order of the Schur form's diagonal,
 * eigenvectors().real() column-major, Francis QR steps, info (0 Success, 1 NumericalIssue, 2 NoConvergence).  NULL = not wanted. */
/* Test hook (ne_triangle): Hp = [J | e0]^T [J | e0] of caller data, in the form the context's switch selects.  E: (P + 1) x rows doubles,
 * evaluation b at E + b * rows, 1 <= P <= 1024 (the panel solve's limit); formed != 0: E holds the columns already (E[0] = e0,
 * E[k + 1] = column k), h is not used.  Hp_out: (P + 1)^2 doubles, column-major.  Above 64 parameters the switch has no say: the columns
 * are formed in place and contracted on the matrix cores, one fused multiply-add per row -- in place means in the hook's private device copy
 * of E, the caller's array is never written. */
int dmsa_debug_normal_equations(dmsa_ctx* ctx, const double* E, int64_t rows, int32_t P, double h, int32_t formed, double* Hp_out);
/* Test hook: out[b] = E_b^T E_b of caller data as the line search computes it (the blocked order of the normal equations).  E: B x rows
 * doubles (host), evaluation b at E + b * rows, 1 <= B <= 65535; P (1 .. 1024) selects the row-block size and, above 64, one fused
 * multiply-add per row.  out: B doubles (host). */
int dmsa_debug_squared_sums(dmsa_ctx* ctx, const double* E, int64_t rows, int32_t B, int32_t P, double* out);
int dmsa_debug_limit_covariance(dmsa_ctx* ctx, const float* cov9, int64_t count, float* out9, float* evals3, float* V9, int32_t* iterations, int32_t* info);
/* Test hooks of csrc/radix_sort.hip on caller data (host arrays): the stable sort of (u64 key, u32 value) pairs on the key bits
 * [0, end_bit) that wide leaf codes go through, and the inclusive (1) / exclusive (0) prefix scan of an int32 array. */
int dmsa_sort_pairs64(dmsa_ctx* ctx, const uint64_t* keys, const uint32_t* values, int64_t n, uint32_t end_bit, uint64_t* keys_sorted, uint32_t* values_sorted);
int dmsa_scan_i32(dmsa_ctx* ctx, const int32_t* in, int64_t n, int32_t inclusive, int32_t* out);

void dmsa_default_debug_options(dmsa_debug_options* o);
/* dmsa_create with explicit switches (`options` may be NULL = defaults); DMSA_DEBUG still overrides by name.  Kept for callers built against
 * the round-5 header: only the fields BEFORE small_voxel (offsetof(dmsa_debug_options, small_voxel) bytes) are read, the ones appended since
 * keep their defaults.  New callers use dmsa_create_ex2 with sizeof(dmsa_debug_options). */
int dmsa_create_ex(int device, uint32_t flags, const dmsa_debug_options* options, dmsa_ctx** out);
/* The same with the size of the caller's struct in bytes (a multiple of 4, at least 4): only that many leading bytes are read, the fields
 * behind them keep their defaults; a size larger than the library's struct is refused (DMSA_ERR_INVALID). */
int dmsa_create_ex2(int device, uint32_t flags, const dmsa_debug_options* options, uint32_t options_bytes, dmsa_ctx** out);
/* The same with switches by name on top of the struct: `named` = "name=value,name=value" or NULL.  The way from code to a switch that has no field
 * in the struct (fit_by_level, batch_stamps, one_readback, next_head, ne_triangle, keys_ahead); DMSA_DEBUG still overrides both. */
int dmsa_create_named(int device, uint32_t flags, const dmsa_debug_options* options, uint32_t options_bytes, const char* named, dmsa_ctx** out);

#ifdef __cplusplus
}
#endif
#endif /* DMSA_DEBUG_H */
