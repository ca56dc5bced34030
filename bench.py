#!/usr/bin/env python
"""bench.py — DMSA iterations/sec on MI355X (BASELINE.json metric), one process per GPU.

A "step" is one DMSA iteration = one pass of the loop body DmsaOptimizer.h:69-144 (2 voxelisations + Gaussian fit +
P+10 forward evaluations + normal equations + line search) on a synthetic 10-scan x 131 072-point sliding window
(+200 000 static map points, 6 control poses, ~1002 dense poses) that is ALREADY RESIDENT in HBM when the timed
region starts.  Early exits are disabled (DMSA_FLAG_FIXED_ITERS) so every step does the same work.

  python bench.py --gpus 1 --steps 20 --warmup 3
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

N > 1: windows are sequentially dependent in a SLAM run, so the window pass shards only as independent problems
("weak" scaling: every rank optimises its own window); the one exchange step of the sharded path — an all-gather of
the optimised poses (RCCL) — is inside the timed region.  value = total iterations of all ranks / max-over-ranks time.

`--workload keyframes` is config 4, the pass that really shards, as a STRONG-scaling workload: ONE ring-buffer map of
--map-frames keyframes (249) is cut into --neighbourhoods (8) neighbourhoods of 32 frames sharing their boundary frames
(sharding.py) whatever N is; rank r keeps the submaps r, r + N, ... resident and optimises them one after the other, and the
timed region ends with ONE all-gather of relative poses + updatePosesFromSubmap for all neighbourhoods on every rank.  N = 1
does the same work as N = 8.  The line carries per-rank time / points / Gaussians and the max / mean ratio (load balance is
what governs this curve: the collective is a few KB).  The same pass runs as a second, separately timed region of the
default (window) workload and is reported there as `keyframe_pass`.  `--map-frames 0` is the weak-scaling layout of rounds
1-3 (one neighbourhood of --frames keyframes per rank, the map grows with N).

`DMSA_BENCH_BACKEND=gloo` rehearses the N > 1 control flow (barriers, gathers, max-over-ranks timing) with more ranks than
GPUs: ranks share devices and the collectives run on CPU tensors (used to test the 2-rank paths on a 1-GPU box).

Rank 0 prints ONE JSON line with the headline metric and `roofline` (correspondence kernel, HIP-event timed on the library stream
during the timed steps themselves).  A plain run does only that: set up, warm up, time --steps steps, print.  `--full` adds what
takes runs of its own: the per-stage breakdown, the PCIe-inclusive calls, the small windows of configs 2 / 5, the sharded keyframe
pass beside the window metric and `cpu_baseline` (the CPU oracle on a bounded sample of the same workload; oracle/ is used here only
as the baseline).

`--dump-outputs DIR` writes what the timed path handed its caller after the last timed step (poses, global points, the report) as
DIR/<name>.npy in float32 / float64; the inputs are seeded, so two builds given the same arguments can be compared file by file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured achievable copy rate
TRAFFIC_FILES = ("r06_traffic.json", "r05_traffic.json", "r04_traffic.json", "r03_traffic.json", "r02_traffic.json")  # newest first
KF_TRAFFIC_FILES = ("r06_traffic_keyframes.json", "r05_traffic_keyframes.json")


def spawn_ranks(n, backend, visible):
    """`python bench.py --gpus N` without a launcher: re-run this command as N ranks under torch.distributed.run (127.0.0.1 rendezvous
    on a free port, one process per GPU) and pass its exit code on."""
    import socket
    import subprocess

    if backend == "nccl" and visible < n:
        print(f"bench.py: --gpus {n} over RCCL needs {n} visible GPUs, found {visible}", file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    print(f"[bench] --gpus {n} without WORLD_SIZE: launching {' '.join(cmd)}", file=sys.stderr)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed iterations (default: a timed region of >= 0.2 s)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="window", choices=["window", "keyframes", "small_imu", "small_rosette"],
                    help="window / keyframes: BASELINE.json configs 3 / 4; small_imu / small_rosette: only the small-window measurement of configs 2 / 5 "
                         "(the reference's everyday problem size), e.g. under rocprofv3")
    ap.add_argument("--scans", type=int, default=10)
    ap.add_argument("--rings", type=int, default=128)
    ap.add_argument("--az", type=int, default=1024)
    ap.add_argument("--static", type=int, default=200_000)
    ap.add_argument("--frames", type=int, default=32, help="keyframes per rank for --workload keyframes --map-frames 0 (weak scaling)")
    ap.add_argument("--map-frames", type=int, default=249, help="keyframes of the ring-buffer map of the sharded keyframe pass (0: weak-scaling layout)")
    ap.add_argument("--neighbourhoods", type=int, default=8, help="neighbourhoods the map is cut into, whatever --gpus is")
    ap.add_argument("--cpu-iters", type=int, default=20, help="oracle iterations timed for cpu_baseline (0 disables)")
    ap.add_argument("--keyframe-steps", type=int, default=10, help="iterations of the secondary sharded-keyframe-pass measurement (0 disables)")
    ap.add_argument("--full", action="store_true", help="also the measurements that take runs of their own: stage breakdown, PCIe-inclusive calls, "
                                                         "small windows, keyframe pass, CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="only the timed region even with --full (the default without it)")
    ap.add_argument("--host-tables", action="store_true", help="build the pose tables on host threads (same bits as the device kernel)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path returned after its last step as DIR/<name>.npy (float32 / float64, at most 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    args.extras = args.full and not args.no_extras
    return args


def main():
    args = parse()
    import torch
    import torch.distributed as dist

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the DMSA path has no CPU fallback")
    # DMSA_BENCH_BACKEND=gloo: rehearse the N > 1 control flow on fewer GPUs than ranks (ranks share devices, collectives on CPU tensors)
    backend = os.environ.get("DMSA_BENCH_BACKEND", "nccl")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: spawn the N ranks ourselves (one process per GPU under torch.distributed.run) instead of
        # quietly measuring one GPU
        raise SystemExit(spawn_ranks(args.gpus, backend, torch.cuda.device_count()))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if backend == "nccl" and world > torch.cuda.device_count():
        raise SystemExit(f"bench.py: {world} ranks over RCCL need {world} visible GPUs, found {torch.cuda.device_count()} "
                         "(DMSA_BENCH_BACKEND=gloo rehearses the control flow on fewer)")
    local_rank = local_rank % torch.cuda.device_count() if backend != "nccl" else local_rank
    torch.cuda.set_device(local_rank)
    coll_dev = f"cuda:{local_rank}" if backend == "nccl" else "cpu"
    if world > 1:
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend=backend)

    # who runs where: every rank's (rank, device) pair and the world size the communicator really has
    placement = [[rank, local_rank]]
    coll_world = 1
    if world > 1:
        coll_world = dist.get_world_size()
        me = torch.tensor([rank, local_rank], dtype=torch.int64, device=coll_dev)
        got = [torch.empty_like(me) for _ in range(world)]
        dist.all_gather(got, me)
        placement = [[int(g[0]), int(g[1])] for g in got]
        if rank == 0:
            print(f"[bench] n_gpus={world} backend={backend} ({'RCCL' if backend == 'nccl' else backend}) collective world size={coll_world} "
                  f"rank->device {placement}", file=sys.stderr)

    from dmsa_lidar_slam_amd import synth
    from dmsa_lidar_slam_amd.api import DmsaOptimizer
    from dmsa_lidar_slam_amd.problems import DmsaOptimSettings

    if args.workload.startswith("small_"):
        if rank == 0:
            outputs = {} if args.dump_outputs else None
            small = small_windows(local_rank, [args.workload[6:]], args.steps, min(args.cpu_iters, 10) if args.extras else 0, calls=args.extras, outputs=outputs)
            if outputs is not None:
                dump_outputs(args.dump_outputs, outputs)
            print(json.dumps({"small_window": small}), flush=True)
        return
    if args.workload == "window":
        prob = synth.window_problem(seed=1 + rank, scans=args.scans, rings=args.rings, az_steps=args.az, num_static=args.static)
        settings = DmsaOptimSettings.sliding_window(num_iter=1)
        wl = f"window{args.scans}x{args.rings * args.az}+static{args.static}"
        n_points = prob.localPoints.shape[0] + prob.staticPoints.shape[0]
    else:
        # config 4: one ring-buffer map cut into `world` neighbourhoods of --frames keyframes sharing one boundary frame;
        # every rank builds the same map (same seed) and keeps only its own submap resident
        from dmsa_lidar_slam_amd.sharding import gather_owned_neighbourhood_poses, neighbourhood_ranges, owned_neighbourhoods

        strong = args.map_frames > 0
        if strong and args.neighbourhoods < world:
            raise SystemExit(f"bench.py: {args.neighbourhoods} neighbourhoods cannot occupy {world} ranks")
        total_frames = args.map_frames if strong else (args.frames - 1) * world + 1
        full_map = bench_keyframe_map(total_frames, rank, world, dist)
        ranges = neighbourhood_ranges(total_frames, args.neighbourhoods if strong else world)
        owned = owned_neighbourhoods(len(ranges), rank, world)
        subs = {nb: full_map.getSubmap(*ranges[nb]) for nb in owned}
        prob = subs[owned[0]]
        settings = DmsaOptimSettings.keyframe_map(num_iter=1)
        wl = f"keyframes{total_frames}/{len(ranges)}x~{prob.localPoints.shape[0] // prob.numFrames}" if strong else f"keyframes{args.frames}x~{prob.localPoints.shape[0] // args.frames}"
        n_points = sum(sb.localPoints.shape[0] for sb in subs.values())

    opt = DmsaOptimizer(device=local_rank, fixed_iters=True, pose_table_host=args.host_tables)
    opt.upload(prob)  # inputs resident in HBM before the timed region
    opts = {}
    if args.workload == "keyframes":  # one context per owned neighbourhood: all of them resident before the timed region
        opts = {owned[0]: opt}
        for nb in owned[1:]:
            opts[nb] = DmsaOptimizer(device=local_rank, fixed_iters=True, pose_table_host=args.host_tables)
            opts[nb].upload(subs[nb])

    def sync_all():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    settings.num_iter = max(1, args.warmup)
    if args.warmup > 0:
        for o in (opts.values() if opts else [opt]):
            o.optimizeResident(settings)
    if world > 1:
        # warm the collective the timed region ends with: the first all-gather on a fresh communicator sets up its xGMI peer
        # connections (tens of ms), which is start-up cost, not part of a step
        w = torch.zeros(64, dtype=torch.float64, device=coll_dev)
        dist.all_gather([torch.empty_like(w) for _ in range(world)], w)
    for o in (opts.values() if opts else [opt]):
        o.timing(reset=True)
    settings.num_iter = args.steps
    per_rank = None
    sync_all()
    t0 = time.perf_counter()
    if args.workload == "keyframes":  # sharded keyframe pass: the owned neighbourhoods one after the other, all-gather + updatePosesFromSubmap on every rank
        reps = {}
        for nb in owned:
            reps[nb] = opts[nb].optimizeResident(settings)
            subs[nb].relOrientations[:], subs[nb].relTranslations[:] = opts[nb].poses()
        t_own = time.perf_counter() - t0
        gather_owned_neighbourhood_poses(full_map, subs, ranges, rank, world, dist, coll_dev)
        rep = reps[owned[0]]
    else:
        rep = opt.optimizeResident(settings)
    if args.workload == "keyframes":
        pass
    elif world > 1:  # independent windows: the exchange step is an all-gather of the optimised poses over RCCL/xGMI
        ro, rt = opt.poses()
        mine = torch.from_numpy(np.concatenate([ro.ravel(), rt.ravel()])).to(coll_dev)
        gathered = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(gathered, mine)
    sync_all()
    elapsed = time.perf_counter() - t0
    tm = opt.timing()
    if args.workload == "keyframes":
        for nb in owned[1:]:  # the roofline figures cover every neighbourhood of this rank
            t_nb = opts[nb].timing()
            for k in ("residual_kernel_ms", "residual_launches", "residual_evaluations", "residual_algorithmic_bytes", "residual_unit_bytes"):
                setattr(tm, k, getattr(tm, k) + getattr(t_nb, k))
        per_rank = rank_telemetry(rank, world, dist, coll_dev, t_own, owned, subs, reps)
    if rep.iterations != args.steps:
        raise SystemExit(f"bench.py: the timed region ran {rep.iterations} iterations, --steps asked for {args.steps}")
    # --dump-outputs: what the caller of the timed path receives after its last step, read back before anything else runs
    if rank == 0 and args.dump_outputs:
        outputs = {}
        if args.workload == "keyframes":
            outputs["rel_orientations"], outputs["rel_translations"] = full_map.relOrientations, full_map.relTranslations
            for nb in owned:
                outputs[f"nb{nb}_global_points"] = opts[nb].globalPoints()
                outputs[f"nb{nb}_report"] = report_array(reps[nb])
        else:
            outputs["rel_orientations"], outputs["rel_translations"] = opt.poses()
            outputs["global_points"] = opt.globalPoints()
            outputs["report"] = report_array(rep)
            if world > 1:
                outputs["gathered_poses"] = torch.stack(gathered).cpu().numpy()
        dump_outputs(args.dump_outputs, outputs)
    # stage breakdown: a second, untimed pass with the per-stage HIP-event timers switched on (they cost GPU idle time)
    stage = None
    if rank == 0 and args.extras:
        opt2 = DmsaOptimizer(device=local_rank, fixed_iters=True, pose_table_host=args.host_tables, stage_timers=True)
        opt2.upload(prob)
        s2 = type(settings)(**{**settings.__dict__, "num_iter": 4})
        opt2.optimizeResident(s2)
        opt2.timing(reset=True)
        r2 = opt2.optimizeResident(s2)
        t2 = opt2.timing()
        k = max(1, r2.iterations)
        stage = {"residual_kernel": round(t2.residual_kernel_ms / k, 4), "voxelize": round(t2.voxelize_ms / k, 4),
                 "gaussian_fit_and_tiles": round(t2.gaussian_fit_ms / k, 4), "pose_tables": round(t2.pose_table_ms / k, 4),
                 "normal_eq": round(t2.normal_eq_ms / k, 4)}
        opt2.close()
    # What a drop-in call costs with the PCIe traffic inside (never `value`): (a) dmsa_optimize_window with host arrays, the whole window
    # uploaded per call; (b) the window resident in a ring (include/dmsa_window_ring.h): one new scan + the static points per call, as
    # DmsaSlam::processPointCloud feeds its ring buffer (DmsaSlam.h:116-204).  Ten iterations per call (num_iter_sliding_window_optim).
    pcie = None
    if rank == 0 and args.workload == "window" and args.extras and hasattr(prob, "scanOffsets"):
        s10 = type(settings)(**{**settings.__dict__, "num_iter": 10})
        o_full = DmsaOptimizer(device=local_rank, fixed_iters=True)
        o_full.optimizeSet(prob.copy(), s10)  # first call: allocations
        t_full = []
        for _ in range(3):
            pc = prob.copy()
            torch.cuda.synchronize()
            t = time.perf_counter()
            o_full.optimizeSet(pc, s10)
            t_full.append(time.perf_counter() - t)
        o_full.close()
        off = prob.scanOffsets
        per_scan = int(np.diff(off).max())
        o_ring = DmsaOptimizer(device=local_rank, fixed_iters=True)
        o_ring.ringCreate(len(off) - 1, per_scan, prob.staticPoints.shape[0], prob.trajTime.size, prob.relOrientations.shape[0])
        for k in range(len(off) - 1):
            o_ring.ringPush(prob.localPoints[off[k]:off[k + 1]], prob.pointStamps[off[k]:off[k + 1]], prob.ringIds[off[k]:off[k + 1]])
        o_ring.uploadFromRing(prob.copy(), prob.t0)
        o_ring.optimizeResident(s10)
        t_ring = []
        for rep_i in range(3):
            k = rep_i % (len(off) - 1)
            pc = prob.copy()
            torch.cuda.synchronize()
            t = time.perf_counter()
            o_ring.ringPush(prob.localPoints[off[k]:off[k + 1]], prob.pointStamps[off[k]:off[k + 1]], prob.ringIds[off[k]:off[k + 1]])  # the window slides by one scan
            o_ring.uploadFromRing(pc, prob.t0)
            o_ring.optimizeResident(s10)
            o_ring.poses()
            t_ring.append(time.perf_counter() - t)
        o_ring.close()
        n_all = prob.localPoints.shape[0]
        cpp = cpp_aos_call(prob, len(off) - 1)
        pcie = {"iterations_per_call": 10,
                "full_upload_call_ms": round(1e3 * min(t_full), 3), "full_upload_it_per_s": round(10 / min(t_full), 1),
                "full_upload_h2d_bytes": int(20 * (n_all + prob.staticPoints.shape[0])),
                "resident_ring_call_ms": round(1e3 * min(t_ring), 3), "resident_ring_it_per_s": round(10 / min(t_ring), 1),
                "resident_ring_h2d_bytes": int(28 * per_scan + 20 * prob.staticPoints.shape[0]),
                # the same call from C++ with the points in the reference's own containers (examples/aos_call_demo.cpp, include/dmsa_aos.h)
                "cpp_aos_call_ms": cpp.get("aos_call_ms") if cpp else None, "cpp_aos_call_poses_only_ms": cpp.get("aos_call_poses_only_ms") if cpp else None,
                "cpp_aos_ring_call_ms": cpp.get("aos_ring_call_ms") if cpp else None, "cpp_flat_call_ms": cpp.get("flat_call_ms") if cpp else None,
                "cpp_host_repack_call_ms": cpp.get("host_repack_call_ms") if cpp else None,
                "cpp_aos_bit_identical_to_flat": (cpp.get("poses_bit_identical") and cpp.get("global_points_bit_identical")) if cpp else None,
                "cpp_aos_h2d_bytes": int(20 * n_all + 16 * prob.staticPoints.shape[0]),
                "note": "wall time of whole calls through the Python ctypes layer, best of 3; (a) dmsa_optimize_window with host arrays, (b) one "
                        "scan pushed into the resident ring + dmsa_window_upload_from_ring + dmsa_optimize_resident + dmsa_get_poses; cpp_*: "
                        "examples/aos_call_demo.cpp, the same 10-iteration call from C++ with one 32-byte-per-point array per scan (the layout of "
                        "pcl::PointCloud<PointStampId>) -- aos: views handed to dmsa_optimize_window_aos + the global points written back into the "
                        "strided container (poses_only: without that write-back), aos_ring: one scan pushed from its container into the resident "
                        "ring, flat: arrays that are already flat, host_repack: the per-point repack a caller of the flat ABI needs"}
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # BASELINE.json also asks for the sharded keyframe pass at 2/4/8 GPUs: measured here as a second, separately timed
    # region (same barrier / max-over-ranks protocol) and reported beside the headline metric, never mixed into `value`.
    keyframe_pass = None
    if args.workload == "window" and args.keyframe_steps > 0 and args.extras:
        keyframe_pass = sharded_keyframe_pass(args, rank, local_rank, world, dist, coll_dev, sync_all)
    # the reference's everyday problem size (configs 2 and 5: five scans of a few thousand points): launch-latency territory
    small = small_windows(local_rank, ["imu", "rosette"], 100, min(args.cpu_iters, 10)) if (rank == 0 and args.workload == "window" and args.extras) else None

    if rank == 0:
        iters = rep.iterations
        units = (len(ranges) if strong else world) if args.workload == "keyframes" else world  # problems optimised per step count
        value = units * iters / elapsed
        launches = max(1, tm.residual_launches)
        evals = max(1, tm.residual_evaluations)
        avg_ms = tm.residual_kernel_ms / launches
        # unit of work = one evaluation, bytes(1) = 16*Mm + 56*M + 48*(n_t+1); a launch processes B units.
        unit_bytes = tm.residual_unit_bytes / evals
        bytes_per_launch = tm.residual_unit_bytes / launches            # per-unit figure x units per launch
        compulsory_per_launch = tm.residual_algorithmic_bytes / launches  # bytes(B): members read once per launch
        achieved = bytes_per_launch / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
        # HBM bytes per launch: PMC counters cannot be read from inside this process, so the figure comes from the committed rocprofv3
        # --pmc passes of this same command (scripts/profile_round.sh -> profiles/rNN_traffic.json) and is labelled as such
        traffic, traffic_source = None, None
        for name in TRAFFIC_FILES:
            try:
                with open(os.path.join(ROOT, "profiles", name)) as f:
                    tj = json.load(f)
                if tj.get("workload") == wl and tj.get("path") == "default":
                    traffic, traffic_source = tj.get("hbm_bytes_per_launch"), f"from_profiles: profiles/{name}"
                    break
            except Exception:
                continue
        # fp32 vector-ALU view of the same launches: 48 flop per member and evaluation, none fusable into FMA
        flops = 48.0 * rep.num_memberships * evals
        valu_tflops = flops / (tm.residual_kernel_ms * 1e-3) / 1e12 if tm.residual_kernel_ms > 0 else 0.0
        out = {
            "metric": "DMSA iterations/sec (10-scan window, 131072 pts/scan)" if args.workload == "window"
                      else "DMSA iterations/sec (sharded keyframe pass, iterations of all neighbourhoods)",
            "value": round(value, 3),
            "unit": "iterations/s",
            "n_gpus": world,
            "steps": iters,
            "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / max(1, iters), 4),
            "higher_is_better": True,
            "scaling": "strong" if (args.workload == "keyframes" and strong) else "weak",
            "vs_baseline": None,
            "dtype": "f32 points/Gaussians, f64 residual sums and normal equations",
            "data": "synthetic",
            "config": {
                "workload": wl,
                "points": int(n_points),
                "control_poses_or_frames": int(prob.relOrientations.shape[0]),
                "params": int(prob.numParams),
                "evaluations_per_iteration": int(prob.numParams) + 10,
                "gaussians": int(rep.num_gaussians),
                "memberships": int(rep.num_memberships),
                "path": "reference-order sums, device pose tables (poses bit-identical to the CPU restatement); the library has one path",
                "rank_device": placement,
                "collective": {"backend": "rccl" if backend == "nccl" else backend, "world_size": coll_world},
                "sharding": (("single GPU" if world == 1 else "independent windows per rank + pose all-gather") if args.workload == "window"
                             else f"{len(ranges)} keyframe neighbourhoods of one {total_frames}-frame map, rank r runs r, r + {world}, ... + one pose all-gather"),
            },
            "roofline": {
                "kernel": "reference-order correspondence kernels (k_residuals_chain<8,true,128> + k_residuals_chain<4,false,32> + k_residuals_small, "
                          "three streams, fork / join by device counters, one HIP-event pair around the batch), B evaluations per launch",
                # what bounds the kernels is vector instruction issue (bound_stated, valu); achieved / peak / frac below are still the brief's
                # HBM-referred figures, and frac_hbm / frac_counters say how far from an HBM bound the launches are
                "bound": "valu",
                # SURVEY 8(d) bytes(B) / t: what a launch of B evaluations MUST move when it reads the members once, over the launch time --
                # the HBM roofline figure proper (the kernels are nowhere near it and cannot be: bound_stated)
                "frac_hbm": round(compulsory_per_launch / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if avg_ms > 0 else None,
                # the brief's figure: per-unit algorithmic bytes (bytes(1)) x units per launch / launch time -- an EFFECTIVE rate, a launch
                # reads the members once per pass for all its evaluations
                "achieved": round(achieved, 2),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4),
                "frac_effective": round(achieved / HBM_PEAK_GBS, 4),
                "frac_compulsory": round(compulsory_per_launch / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if avg_ms > 0 else None,
                # HBM bytes the PMC passes counted (profiles/r02_traffic.json), same launch time
                "frac_counters": round(traffic / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if (traffic and avg_ms > 0) else None,
                "traffic": traffic,
                "traffic_source": traffic_source,
                "avg_launch_ms": round(avg_ms, 5),
                "launches": int(tm.residual_launches),
                "evaluations": int(tm.residual_evaluations),
                "algorithmic_bytes_per_evaluation": round(unit_bytes, 1),
                "algorithmic_bytes_per_launch": round(bytes_per_launch, 1),
                "compulsory_bytes_per_launch": round(compulsory_per_launch, 1),
                "us_per_evaluation": round(1e3 * tm.residual_kernel_ms / evals, 3),
                "bound_stated": "not HBM: vector instruction issue (the three tier kernels use 86 - 89 % of the issue slots; in both batches the "
                                "throughput tier ends last, the latency tier's 110 long Gaussians keep ~220 compute units busy beside it: "
                                "profiles/r06_iteration_timeline.txt).  A launch evaluates B pose tables on members it reads once per pass, so "
                                "`achieved` / `frac` are an effective rate; the HBM fractions are frac_compulsory and frac_counters",
                # the peak that applies: one wave64 fp32 instruction per SIMD every 4 cycles, no FMA (the reference rounds every product and
                # sum on its own) and no packed issue (a wave64 v_pk_* occupies the SIMD for two passes): 1024 SIMDs x 64 lanes / 4 cycles x 2.4 GHz
                "valu": {"achieved_tflops": round(valu_tflops, 2), "peak_tflops_scalar_no_fma": 39.3,
                         "frac": round(valu_tflops / 39.3, 4)},
            },
            "per_rank": per_rank,
            "stage_ms_per_step": stage,
            "keyframe_pass": keyframe_pass,
            "small_window": small,
            "pcie_inclusive": pcie,
        }
        if world == 1 and args.cpu_iters > 0 and args.extras:
            out["cpu_baseline"] = cpu_baseline(prob, settings, args.cpu_iters, args.workload)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def bench_keyframe_map(total_frames, rank, world, dist):
    """The synthetic ring-buffer map of config 4 (k-NN normals included: ~14 s for 249 frames on one host thread), generated ONCE -- by
    rank 0, cached as a flat dump (dmsa_lidar_slam_amd/dump.py) that the other ranks and later runs read."""
    import tempfile

    from dmsa_lidar_slam_amd import dump, synth

    # the cache is keyed by what generates the map -- frame count, seed, arc and the source of the generator itself -- so a change of
    # synth.keyframe_problem or a stale / foreign file cannot feed different data into the reported numbers
    import hashlib
    import inspect

    seed, arc = 1, 2 * np.pi * total_frames / 256.0
    key = hashlib.sha1((inspect.getsource(synth) + inspect.getsource(dump) + f"|{total_frames}|{seed}|{arc!r}").encode()).hexdigest()[:12]
    path = os.path.join(tempfile.gettempdir(), f"dmsa_bench_keyframe_map_{total_frames}_{key}.bin")
    if rank == 0 and not os.path.exists(path):
        m = synth.keyframe_problem(seed=seed, frames=total_frames, arc=arc)
        dump.write_keyframe_map(path + f".{os.getpid()}", m)
        os.replace(path + f".{os.getpid()}", path)
    if world > 1:
        dist.barrier()
    return dump.read_keyframe_map(path)


def rank_telemetry(rank, world, dist, coll_dev, t_own, owned, subs, reps):
    """What governs the scaling curve of the sharded keyframe pass: every rank's own time (before the collective), points, Gaussians."""
    import torch

    mine = [float(rank), 1e3 * t_own, float(len(owned)), float(sum(subs[nb].localPoints.shape[0] for nb in owned)),
            float(sum(reps[nb].num_gaussians for nb in owned)), float(sum(reps[nb].num_memberships for nb in owned))]
    rows = [mine]
    if world > 1:
        t = torch.tensor(mine, dtype=torch.float64, device=coll_dev)
        got = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(got, t)
        rows = [g.cpu().tolist() for g in got]
    ms = [r[1] for r in rows]
    return {"ranks": [{"rank": int(r[0]), "ms": round(r[1], 3), "neighbourhoods": int(r[2]), "points": int(r[3]), "gaussians": int(r[4]), "memberships": int(r[5])}
                      for r in rows],
            "max_over_mean_ms": round(max(ms) / (sum(ms) / len(ms)), 4), "slowest_rank": int(rows[int(np.argmax(ms))][0])}


def sharded_keyframe_pass(args, rank, local_rank, world, dist, coll_dev, sync_all):
    """BASELINE.json config 4 as a strong-scaling workload: ONE ring-buffer map of --map-frames keyframes cut into --neighbourhoods
    neighbourhoods whatever the world size; rank r optimises neighbourhoods r, r + world, ... one after the other (full optimizeSet each),
    ONE all-gather of relative poses, updatePosesFromSubmap for every neighbourhood on every rank."""
    import torch

    from dmsa_lidar_slam_amd.api import DmsaOptimizer
    from dmsa_lidar_slam_amd.problems import DmsaOptimSettings
    from dmsa_lidar_slam_amd.sharding import gather_owned_neighbourhood_poses, neighbourhood_ranges, owned_neighbourhoods

    strong = args.map_frames > 0 and args.neighbourhoods >= world
    total_frames = args.map_frames if strong else (args.frames - 1) * world + 1
    full_map = bench_keyframe_map(total_frames, rank, world, dist)
    ranges = neighbourhood_ranges(total_frames, args.neighbourhoods if strong else world)
    owned = owned_neighbourhoods(len(ranges), rank, world)
    subs = {nb: full_map.getSubmap(*ranges[nb]) for nb in owned}
    s = DmsaOptimSettings.keyframe_map(num_iter=2)
    opts = {}
    for nb in owned:
        opts[nb] = DmsaOptimizer(device=local_rank, fixed_iters=True)
        opts[nb].upload(subs[nb])
        opts[nb].optimizeResident(s)
    s.num_iter = args.keyframe_steps
    for o in opts.values():
        o.timing(reset=True)
    sync_all()
    t0 = time.perf_counter()
    reps = {}
    for nb in owned:
        reps[nb] = opts[nb].optimizeResident(s)
        subs[nb].relOrientations[:], subs[nb].relTranslations[:] = opts[nb].poses()
    t_own = time.perf_counter() - t0
    gather_owned_neighbourhood_poses(full_map, subs, ranges, rank, world, dist, coll_dev)
    sync_all()
    elapsed = time.perf_counter() - t0
    # roofline of the pass's dominant kernels (the correspondence batches of this rank's neighbourhoods), HIP events on their streams
    acc = {k: 0.0 for k in ("residual_kernel_ms", "residual_launches", "residual_evaluations", "residual_algorithmic_bytes", "residual_unit_bytes")}
    for o in opts.values():
        t_nb = o.timing()
        for k in acc:
            acc[k] += getattr(t_nb, k)
    launches, evals = max(1.0, acc["residual_launches"]), max(1.0, acc["residual_evaluations"])
    avg_ms = acc["residual_kernel_ms"] / launches
    eff = acc["residual_unit_bytes"] / launches / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
    comp = acc["residual_algorithmic_bytes"] / launches / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
    memb = sum(int(r.num_memberships) for r in reps.values())
    flops = 48.0 * memb / max(1, len(reps)) * evals  # 48 flop per member and evaluation (mean memberships of this rank's neighbourhoods)
    valu = flops / (acc["residual_kernel_ms"] * 1e-3) / 1e12 if acc["residual_kernel_ms"] > 0 else 0.0
    # HBM bytes per launch from the committed PMC passes of one neighbourhood of this shape (scripts/kf_pmc.sh -> profiles/rNN_traffic_keyframes.json)
    traffic, traffic_source = None, "no PMC pass for this workload"
    for name in KF_TRAFFIC_FILES:
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                traffic, traffic_source = json.load(f).get("hbm_bytes_per_launch"), f"from_profiles: profiles/{name}"
            break
        except Exception:
            continue
    roofline = {"kernel": "reference-order correspondence kernels of the neighbourhoods of rank 0 (B = P + 1 = 187 and B = 9 evaluations per launch)",
                "bound": "valu", "achieved": round(eff, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(eff / HBM_PEAK_GBS, 4),
                "frac_compulsory": round(comp / HBM_PEAK_GBS, 4),
                "frac_counters": round(traffic / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if (traffic and avg_ms > 0) else None,
                "traffic": traffic, "traffic_source": traffic_source,
                "avg_launch_ms": round(avg_ms, 5), "launches": int(launches), "evaluations": int(evals),
                "algorithmic_bytes_per_launch": round(acc["residual_unit_bytes"] / launches, 1),
                "compulsory_bytes_per_launch": round(acc["residual_algorithmic_bytes"] / launches, 1),
                "share_of_pass": round(acc["residual_kernel_ms"] * 1e-3 / max(t_own, 1e-9), 4),
                "valu": {"achieved_tflops": round(valu, 2), "peak_tflops_scalar_no_fma": 39.3, "frac": round(valu / 39.3, 4)},
                "bound_stated": "an effective rate (a launch evaluates B pose tables on members it reads once per pass); the kernels are bound by "
                                "vector issue, and the pass as a whole by its dependent single-workgroup kernels: LM solve 223 us of 1.1 ms per "
                                "neighbourhood iteration (DESIGN.md, where the time is)"}
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    per_rank = rank_telemetry(rank, world, dist, coll_dev, t_own, owned, subs, reps)
    for o in opts.values():
        o.close()
    rep = reps[owned[0]]
    return {"metric": "DMSA iterations/sec (sharded keyframe pass, iterations of all neighbourhoods)", "value": round(len(ranges) * rep.iterations / elapsed, 3),
            "unit": "iterations/s", "n_gpus": world, "steps": int(rep.iterations), "ms_per_step": round(1e3 * elapsed / max(1, rep.iterations), 4),
            "ms_per_neighbourhood_iteration": round(1e3 * elapsed / max(1, rep.iterations) / max(1, len(owned)), 4),
            "scaling": "strong" if strong else "weak", "frames_total": int(total_frames), "neighbourhoods": len(ranges),
            "neighbourhoods_per_rank": len(owned), "params_per_neighbourhood": int(subs[owned[0]].numParams), "roofline": roofline, "per_rank": per_rank,
            "exchange": "one all-gather of ceil(neighbourhoods / ranks) x 32 x 6 doubles per rank" if world > 1 else "none (single GPU)"}


def cpp_aos_call(prob, num_scans):
    """examples/aos_call_demo: a 10-iteration drop-in call from C++ with one 32-byte-per-point array per scan (the layout of
    pcl::PointCloud<PointStampId>), views handed to dmsa_optimize_window_aos, global points written back into the strided container."""
    import subprocess
    import tempfile

    from dmsa_lidar_slam_amd import dump

    exe = os.path.join(ROOT, "examples", "aos_call_demo")
    if not os.path.exists(exe):
        return None
    path = os.path.join(tempfile.gettempdir(), f"dmsa_bench_window_{os.getpid()}.bin")
    try:
        dump.write_window_problem(path, prob)
        r = subprocess.run([exe, path, str(num_scans), "10", "3"], capture_output=True, text=True, timeout=300)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(f"[bench] aos_call_demo failed ({r.returncode}): {r.stderr[-500:]}\n")
            return None
        return json.loads(lines[-1])
    finally:
        if os.path.exists(path):
            os.remove(path)


def small_windows(device, which, steps, cpu_iters, calls=True, outputs=None):
    """Configs 2 and 5 of BASELINE.json at their real shapes (config/slam_settings.yaml:6,24-28, config/livox.yaml:43 of the reference): five
    scans of ~3 000 points after preProcess + 10^4 static map points with IMU rows ('imu', Hilti-like, 32 rings), and five rosette
    scans of 24 000 points without IMU ('rosette', Livox-like).  At this size an iteration is ~60 dependent launches of microseconds each:
    the GPU is launch-latency bound, and the number next to the CPU oracle's says how much of the headline ratio survives."""
    from dmsa_lidar_slam_amd import synth
    from dmsa_lidar_slam_amd.api import DmsaOptimizer
    from dmsa_lidar_slam_amd.problems import DmsaOptimSettings
    import torch

    out = {}
    for name in which:
        if name == "imu":
            prob = synth.window_problem(seed=5, scans=5, rings=32, az_steps=96, num_static=10_000, use_imu=True)
            settings = DmsaOptimSettings.sliding_window(use_imu=True, num_iter=1)
            shape = "5 x 3 072 points (32 rings) + 10 000 static, IMU rows"
        else:
            prob = synth.rosette_window_problem(seed=2, scans=5, pts_per_scan=24_000, num_static=20_000)
            settings = DmsaOptimSettings.sliding_window(num_iter=1)
            shape = "5 x 24 000 rosette points + 20 000 static, no IMU"
        opt = DmsaOptimizer(device=device, fixed_iters=True)
        opt.upload(prob)
        settings.num_iter = 5
        opt.optimizeResident(settings)
        opt.timing(reset=True)
        settings.num_iter = steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = opt.optimizeResident(settings)
        dt = time.perf_counter() - t0
        if outputs is not None:  # --dump-outputs: what this timed call returned, before the drop-in calls below move the poses on
            outputs[f"{name}_rel_orientations"], outputs[f"{name}_rel_translations"] = opt.poses()
            outputs[f"{name}_global_points"] = opt.globalPoints()
            outputs[f"{name}_report"] = report_array(rep)
        # one call of ten iterations with the upload inside: what DmsaSlam::processPointCloud pays per scan at this size
        s10 = type(settings)(**{**settings.__dict__, "num_iter": 10})
        call_ms = []
        for _ in range(5 if calls else 0):
            pc = prob.copy()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            opt.optimizeSet(pc, s10)
            call_ms.append(time.perf_counter() - t1)
        opt.close()
        entry = {"shape": shape, "points": int(prob.localPoints.shape[0] + prob.staticPoints.shape[0]), "params": int(prob.numParams),
                 "gaussians": int(rep.num_gaussians), "memberships": int(rep.num_memberships),
                 "value": round(rep.iterations / dt, 2), "unit": "iterations/s", "ms_per_step": round(1e3 * dt / max(1, rep.iterations), 4),
                 "drop_in_call_10_iterations_ms": round(1e3 * min(call_ms), 3) if call_ms else None}
        if cpu_iters > 0:
            cb = cpu_baseline(prob, settings, cpu_iters, "window", parallel=False)
            entry["cpu_oracle_it_per_s"] = cb["value"]
            entry["gpu_over_cpu"] = round(entry["value"] / cb["value"], 1) if cb["value"] > 0 else None
        out[name] = entry
    out["note"] = ("launch-latency bound: see profiles/r06_small_window_*.txt for the launch count and the sum of kernel time against wall time per "
                   "iteration (DESIGN.md 6.3)")
    return out


REPORT_FIELDS = ("iterations", "stop_reason", "num_gaussians", "num_gaussians_l1", "num_memberships", "error0", "last_step_norm",
                 "last_line_search_k", "evaluations")
DUMP_BUDGET_BYTES = 60_000_000  # under 64 MB however counted, .npy headers included


def report_array(rep):
    """The dmsa_report of a call as float64, fields in REPORT_FIELDS order (every integer field is exact in a double)."""
    return np.array([float(getattr(rep, f)) for f in REPORT_FIELDS], np.float64)


def dump_outputs(directory, arrays):
    """--dump-outputs: one DIR/<name>.npy per array, float64 kept, everything else as float32.  Above DUMP_BUDGET_BYTES in all, every
    array of more than 1 MB keeps the same share of its rows, chosen by a generator seeded with 0 (sorted), so that two runs of the
    same arguments write the same rows."""
    arrays = {k: np.ascontiguousarray(v, np.float64 if np.asarray(v).dtype == np.float64 else np.float32) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_BUDGET_BYTES:
        small = sum(a.nbytes for a in arrays.values() if a.nbytes <= 1 << 20)
        share = (DUMP_BUDGET_BYTES - small) / (total - small)
        for k, a in arrays.items():
            if a.nbytes > 1 << 20:
                keep = max(1, int(a.shape[0] * share))
                arrays[k] = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
    os.makedirs(directory, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(directory, f"{k}.npy"), a)


def cpu_baseline(prob, settings, iters, workload, parallel=True):
    """The CPU oracle (the repo's restatement of the reference's single-threaded -O2 loop; the reference itself cannot
    be built here) timed on the SAME workload for a bounded number of iterations."""
    from oracle import oracle_py as orc

    s = type(settings)(**{**settings.__dict__, "num_iter": iters})
    fn = orc.optimize_window if workload == "window" else orc.optimize_keyframes

    def timed(threads):
        orc.set_threads(threads)
        try:
            p = prob.copy()
            t0 = time.perf_counter()
            rep, _, _ = fn(p, s, fixed_iters=True)
            return rep.iterations, time.perf_counter() - t0
        finally:
            orc.set_threads(1)

    it1, dt1 = timed(1)
    if not parallel:
        return {"value": round(it1 / dt1, 4), "unit": "iterations/s", "cores": 1, "kind": "port"}
    threads = max(1, min(32, os.cpu_count() or 1))
    itp, dtp = timed(threads)
    return {
        "value": round(it1 / dt1, 4),
        "unit": "iterations/s",
        "cores": 1,
        "kind": "port",
        "sample": f"{it1} iterations of the same {workload} workload ({dt1:.1f} s), g++ -O2, 1 thread "
                  "(the reference is effectively single-threaded, DmsaOptimizer.h:56-57)",
        "parallel_variant": {"value": round(itp / dtp, 4), "cores": threads,
                             "note": "same oracle with the forward differences / line-search trials spread over OpenMP threads "
                                     f"({itp} iterations, {dtp:.1f} s); voxelisation and Gaussian fit stay serial as in the reference"},
    }


if __name__ == "__main__":
    try:
        main()
    except Exception as e:  # noqa: BLE001
        # A tool that serialises kernels across queues (hardware counter collection) can starve a device-side stream dependency
        # (csrc/dev_sync.h): the library then fails loudly instead of hanging.  A single-process run is repeated with HIP events.
        if ("stream dependency timed out" in str(e) and int(os.environ.get("WORLD_SIZE", "1")) == 1
                and "device_sync=0" not in os.environ.get("DMSA_DEBUG", "")):
            sys.stderr.write("[bench] device-side stream dependency timed out -- repeating with DMSA_DEBUG=device_sync=0 (HIP events)\n")
            os.environ["DMSA_DEBUG"] = ",".join(x for x in (os.environ.get("DMSA_DEBUG", ""), "device_sync=0") if x)
            main()
        else:
            raise
