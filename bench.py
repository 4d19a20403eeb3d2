#!/usr/bin/env python3
"""bench.py -- frames/sec of the stereo front-end hot path (LK pyramid update,
forward-backward LK, key-frame detect + stereo LK + triangulation) on MI355X,
plus local-BA ms/iteration, against the HBM roofline, with the CPU oracle timed
beside it.

    python bench.py --gpus N --steps K --warmup W [--full | --only leg[,leg...]] [--dump-outputs DIR]

One process per GPU (a launcher's WORLD_SIZE / RANK are honoured; without one,
`--gpus N` starts the N rank processes itself).  A step = ONE KEY-FRAME PERIOD
(KF_EVERY = 5 frames, the first of them a key-frame) of EACH of S lock-stepped,
independent synthetic KITTI-05-shaped stereo streams (370 x 1226, 1000
keypoints) through the hot path -- every timed step is the same work: 5 left
pyramid builds + 5 temporal matches + 1 cull / detect / right build / stereo
match / triangulation, every launch shared by the S streams, keypoint lists
resident in HBM (slam_kpset_*).  The frames START IN PINNED HOST MEMORY as the
decoder's 8-bit images and are copied to the GPU inside the timed loop; all
arithmetic is Float64 and every plane bit-exact.  value = frames/s over all
streams and GPUs = S * KF_EVERY * K / seconds.  N>1 = N independent replicas
(the front-end does not shard: SURVEY 8e) -> weak scaling, no collective in the
data path.  Rank 0 prints ONE compact JSON line (< 4 KB) as its LAST stdout line;
the full record goes to bench_detail.json and stderr.

A plain run measures the headline alone: set-up, warm-up, the K timed steps, the
line.  `--full` runs every leg below -- the other workloads, precisions and
configurations, the rooflines (with their own runs of the build), the CPU baseline
and the oracle checks of the timed run.  `--only` runs the named legs the way
`--full` does (for profiling one population of kernels at a time):
  single, tolerance, headline, tolbatch, ingest, sweep, host_protocol, configs,
  ba, ba_sharded, pose, cpu
`--dump-outputs DIR` writes what the headline's last timed step left for its
caller as DIR/<name>.npy (float64; dump_outputs below).
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

from benchlib.common import (KF_EVERY, RIGHT_TARGET_ONLY, CULL_FRACTION, N_FRAMES, HBM_PEAK_GBS, HBM_ACHIEVABLE_GBS,      # noqa: E402,F401
                             frame_sequence, frame_sequence_n, pyramid_bytes, iir_rows_bytes)
from benchlib.backends import Stream, GpuBackend, GpuPeriodBackend, CpuBackend                                           # noqa: E402,F401
from benchlib.lockstep import run_lockstep, run_lockstep_kpset, kernel_spans, make_workload, WORKLOADS, leg_ctx, peek, BAWorker, BA_WINDOW_SHAPES   # noqa: E402,F401
from benchlib.checkers import replay_stream_on_oracle                                                                    # noqa: E402
from benchlib.report import compact_line, write_detail, frame_and_lk_rooflines, newest_pmc                               # noqa: E402


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: N fresh processes, one per GPU (this process never initialises HIP).
    A rank that fails takes its siblings with it (they would wait in a collective for ever), and the whole job has a deadline."""
    import socket
    import subprocess
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    procs = []
    one_gpu = os.environ.get("SLAM_BENCH_ONE_GPU") is not None      # test hook: all ranks share GPU 0, collectives over gloo (scripts/two_rank_one_gpu.sh)
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0" if one_gpu else str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        if one_gpu:
            env["SLAM_BENCH_BACKEND"] = "gloo"
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    part = os.path.join(ROOT, "bench_headline_partial.json")
    if os.path.exists(part):                                 # a stale record of an earlier run must never be printed for this one
        os.remove(part)
    deadline = time.time() + float(os.environ.get("SLAM_BENCH_SPAWN_TIMEOUT_S", "3600"))
    t_start = time.time() - 1.0
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            code = p.poll()
            if code is not None:
                live.remove(p)
                rc = max(rc, abs(code))
        if live and (rc != 0 or time.time() > deadline):
            for p in live:                                   # exactly the processes started above
                p.kill()
            for p in live:
                p.wait()
            rank0_done = procs[0] not in live and procs[0].returncode == 0     # rank 0 already printed its full line: a second, degraded one would be what `tail -1` reads
            if not rank0_done and os.path.exists(part) and os.path.getmtime(part) >= t_start:      # rank 0 had measured the headline before a rank was lost: one line, marked
                try:
                    j = json.load(open(part))
                    j["leg_error"] = {"after_leg": "headline", "error": f"a rank process exited with status {rc or 124}: the remaining ranks were stopped; the line is rank 0's headline as measured before that"}
                    print(json.dumps(j, separators=(",", ":")), flush=True)
                except Exception:                              # noqa: BLE001
                    pass
            return rc or 124
        time.sleep(0.2)
    if rc == 0 and os.path.exists(part):
        os.remove(part)
    return rc


LEGS = ("single", "tolerance", "headline", "tolbatch", "ingest", "sweep", "host_protocol", "configs", "ba", "ba_sharded", "pose", "cpu")



def ba_windows(syn):
    """The BA windows SURVEY 8d / BASELINE name.  P5: the reference's own shape -- at most 5 free key-frames and many
    constant observers (estimator.jl:327-331, :163-229): 25 poses of which the 20 oldest are constant, O ~ 8 k.
    P20 / P50 / P100: every point seen by 10 consecutive key-frames.  P50_loop: the 50-KF window with loop-closure observations
    (1500 points of the first 5 key-frames re-observed by the last 5): half-bandwidth 48 in key-frame order (a ring), 18 in the
    folded order slam_local_ba solves it in.  P26_dense: every point seen by 24 consecutive key-frames -- half-bandwidth 23 in any
    order: the non-banded general path (pair lists + tiled Cholesky)."""
    w = {}
    s = syn.ba_scene(P=25, M=800, seed=5, n_const=20); w["P5_free_20_const"] = s
    w["P20"] = syn.ba_scene(P=20, M=4000, seed=6)
    w["P50"] = syn.ba_scene(P=50, M=10000, seed=7)
    w["P100"] = syn.ba_scene(P=100, M=40000, seed=8)
    w["P50_loop"] = syn.ba_scene_loop(P=50, M=10000, seed=7, n_loop=1500)
    w["P26_dense"] = syn.ba_scene(P=26, M=5200, seed=9, obs_per_point=24)
    return w


PLANE_SAMPLE = 1 << 16          # elements kept per plane and level in --dump-outputs (levels 0 and 1 of a 370 x 1226 frame are larger)


def dump_outputs(d, head):
    """--dump-outputs: what the headline loop's last frame step left for its caller -- every stream's keypoint list (positions,
    3-D flags, triangulated points, ids) and the S list lengths -- and all six planes of every level of the current left pyramids
    of the snapshot streams (0 and S - 1), each plane a fixed, seeded sample of PLANE_SAMPLE elements where it is larger (the
    planes of all S streams are GBs).  Float64 .npy files, at most 64 MB together."""
    lists = head["lists"]
    arrays = {"keypoint_counts": np.array([len(k["yx"]) for k in lists], dtype=np.float64),
              "keypoints_yx": np.concatenate([k["yx"] for k in lists]),
              "keypoints_is_3d": np.concatenate([k["is_3d"] for k in lists]).astype(np.float64),
              # a keypoint's point is defined once it is 3-D (fresh detections carry whatever the slot held)
              "keypoints_xyz": np.concatenate([np.where(k["is_3d"][:, None], k["xyz"], 0.0) for k in lists]),
              "keypoint_ids": np.concatenate([k["ids"] for k in lists]).astype(np.float64)}
    for s_, sn in sorted(head["snapshot"].items()):
        for (nm, l), a in sorted(sn["planes"].items()):
            a = np.ravel(a)
            if a.size > PLANE_SAMPLE:
                a = a[np.sort(np.random.default_rng(l).choice(a.size, PLANE_SAMPLE, replace=False))]
            arrays[f"left_pyramid_s{s_}_{nm}_l{l}"] = np.asarray(a, dtype=np.float64)
    total = sum(a.nbytes for a in arrays.values())
    assert total <= 64e6, total
    os.makedirs(d, exist_ok=True)
    if not os.path.exists(os.path.join(d, ".gitignore")):            # a dump inside a checkout stays out of git status, wherever it is
        with open(os.path.join(d, ".gitignore"), "w") as f:
            f.write("*\n")
    for name, a in arrays.items():
        np.save(os.path.join(d, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=60, help="timed steps; one step = one key-frame period (5 frames) of each of the S streams")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--full", action="store_true", help="run every leg (default: the headline alone, without its rooflines)")
    ap.add_argument("--only", type=str, default="", help="comma-separated legs to run as --full runs them: " + ", ".join(LEGS))
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the headline's last step computed "
                    "as DIR/<name>.npy (float64, <= 64 MB in all; identical inputs for identical arguments)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the cpu_baseline leg (and the oracle parity checks that live in it)")
    ap.add_argument("--no-ba", action="store_true", help="skip the BA and pose measurements")
    ap.add_argument("--streams", type=int, default=128, help="S: independent stereo streams per GPU advancing in lock-step (one batch of S frames per frame step); "
                    "128 = the library's batch limit: every launch is shared by more frames (same-box sweep 32 / 64 / 96 / 128: 18.6 / 20.8 / 21.5 / 22.1 k frames/s)")
    ap.add_argument("--no-tolerance", action="store_true", help="skip the tolerance-mode measurements")
    ap.add_argument("--no-sweep", action="store_true", help="skip the streams-per-GPU sweep legs (S = 32 / 64 / 96 at the default 128)")
    ap.add_argument("--no-configs", action="store_true", help="skip the other BASELINE shapes (kitti00_2000, euroc_mono, fhd_4000)")
    args = ap.parse_args()
    full = args.full or bool(args.only)
    legs = set(x for x in args.only.split(",") if x) or (set(LEGS) if args.full else {"headline"})
    unknown = legs - set(LEGS)
    if unknown:
        raise SystemExit(f"unknown leg(s) {sorted(unknown)}; known: {LEGS}")
    if args.dump_outputs and "headline" not in legs:
        raise SystemExit("--dump-outputs writes the headline's outputs: the headline leg must run")
    if args.no_cpu: legs.discard("cpu")
    if args.no_ba: legs -= {"ba", "ba_sharded", "pose"}
    if args.no_tolerance: legs.discard("tolerance")
    if args.no_sweep: legs.discard("sweep")
    if args.no_configs: legs.discard("configs")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: this process has not touched the GPU; it starts N fresh rank processes (one per GPU,
        # the same environment the torch.distributed.run launcher gives them), forwards rank 0's line and exits with their status
        raise SystemExit(spawn_ranks(args))

    # The single-stream legs (latency views) and the lock-stepped legs want different process states: once a stream of another priority
    # class exists (the headline's tracking context) the default-class single-stream legs lose ~40 %, and the dozen contexts the
    # single-stream legs create and destroy shift the runtime's stream -> hardware-queue placement of the headline's four streams
    # (-2.5 % on `value`, same-box A/B).  So this process -- before it touches the GPU -- runs them in a CHILD process of their own
    # (a fresh process per GPU; at N > 1 every rank does so for its GPU and the slowest rank counts) and merges their part of the line.
    child_part = None
    if legs & {"single", "tolerance"} and os.environ.get("SLAM_BENCH_CHILD") is None and legs - {"single", "tolerance"}:
        import subprocess
        sub = sorted(legs & {"single", "tolerance"})
        env = dict(os.environ, SLAM_BENCH_CHILD="1", WORLD_SIZE="1", RANK="0")
        cmd = [sys.executable, os.path.abspath(__file__), "--only", ",".join(sub), "--steps", str(args.steps), "--warmup", str(args.warmup), "--streams", str(args.streams)]
        try:
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=900)
            child_part = json.loads(r.stdout.strip().split("\n")[-1])
        except Exception as ex:                                   # the optional legs never cost the line
            child_part = {"single_stream": {"error": repr(ex)[:200]}}
        legs -= {"single", "tolerance"}

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback)")
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("SLAM_BENCH_BACKEND", "nccl")      # "gloo" only to exercise the N>1 logic on a 1-GPU box
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    if os.environ.get("SLAM_BENCH_KILL_RANK") == str(rank) and world > 1:      # test hook (tests/test_gpu_two_rank_bench.py): this rank dies before its first leg
        os._exit(7)
    import slam_jl_amd as slam
    from slam_jl_amd import synthetic as syn
    ctx = None                                               # the context of the BA / pose legs: created when they start -- an idle stream created up
                                                             # front shifts the runtime's stream -> hardware-queue placement of the headline's four (-4 %, same-box A/B)
    dev = torch.device("cuda", local_rank)
    S = args.streams
    wl = make_workload(slam, syn, "kitti05_1000", seed=rank, streams=S)
    H, W, params, extractor, levels = wl["H"], wl["W"], wl["params"], wl["extractor"], wl["levels"]
    left, right, flows, disparity = wl["left"], wl["right"], wl["flows"], wl["disparity"]
    frame_steps = args.steps * KF_EVERY
    fails = []
    pose_fails = []                                          # a loop whose recovered poses are wrong measured a different workload: leg_error

    progress = {"last_done": "start"}

    def leg_done(tag):
        """every leg leaves the device clean: an asynchronous HIP error is reported against the leg that caused it"""
        try:
            torch.cuda.synchronize()
        except Exception as ex:
            raise RuntimeError(f"bench leg '{tag}' left a HIP error: {ex}") from ex
        progress["last_done"] = tag
        if os.environ.get("SLAM_BENCH_INJECT_ERROR") == tag:     # test hook for the containment below
            raise RuntimeError(f"injected after leg '{tag}'")

    def max_over_ranks(dt):
        if world > 1:
            tt = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            return float(tt[0])
        return dt

    out = {
        "metric": "frames/sec KITTI-05 stereo @1k kpts; local-BA ms/iter for 50-KF window",
        "value": None, "unit": "frames/sec",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": None, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic", "legs": sorted(legs),
    }

    if child_part is not None:
        for key in ("single_stream", "tolerance_mode"):
            if key in child_part:
                out[key] = dict(child_part[key])
        if world > 1:                                            # one stream per GPU: the slowest GPU counts, times the number of GPUs
            for key, sub_ in (("single_stream", None), ("tolerance_mode", "single_stream")):
                node = out.get(key, {}) if sub_ is None else out.get(key, {}).get(sub_, {})
                if "value" in node:
                    tt = torch.tensor([float(node["value"])], dtype=torch.float64, device=dev)
                    dist.all_reduce(tt, op=dist.ReduceOp.MIN)
                    node["value"] = float(tt[0]) * world
        out["legs"] = sorted(set(out["legs"]) | ({"single"} if "single_stream" in child_part else set()) | ({"tolerance"} if "tolerance_mode" in child_part else set()))
        out["single_stream_legs_in_child_process"] = True
    # The single-stream legs (latency views) run FIRST: once a stream of another priority class exists in the process (the headline legs
    # create one for their tracking context) the runtime schedules the default-class queues differently and these latency-bound legs
    # lose ~40 % (measured: 2 260 -> 1 400 frames/s); a deployment picks one configuration or the other, the bench measures each in its own.
    if legs & {"single", "tolerance"}:
        # Julia layout: column-major H x W  ==  row-major (W, H) tensor
        left_dev = [torch.from_numpy(np.ascontiguousarray(im.T)).to(dev) for im in left]
        right_dev = [torch.from_numpy(np.ascontiguousarray(im.T)).to(dev) for im in right]
        torch.cuda.synchronize()
        n1 = min(frame_steps, 300)
        seq = frame_sequence(args.warmup * KF_EVERY + n1 + 202)   # the ping-pong sequence is periodic
        w1 = max(args.warmup, 2) * KF_EVERY

        AH = 2 * KF_EVERY                                        # frames of lookahead the sequence provides to the build pipeline

        def one_stream(fast, ahead=1, period=False):
            sp = int(os.environ.get("SLAM_BENCH_SINGLE_PRIO", "0"))          # scheduling class of the tracking context (experiment)
            c3 = [slam.Context(local_rank, priority=sp)] + [slam.Context(local_rank) for _ in range(2 + max(ahead - 1, 0))]
            if period:
                be = GpuPeriodBackend(slam, c3[0], c3[1], H, W, left_dev, right_dev, params, extractor, KF_EVERY)
            else:
                be = GpuBackend(slam, c3[0], c3[1], c3[2], H, W, left_dev, right_dev, params, extractor, fast=fast, ahead=ahead, extra_build_ctx=c3[3:])
            stream = Stream(be, flows, disparity, seed=rank)
            be.prime(seq[0])
            for i in range(w1):
                stream.step(seq[i], seq[i + 1], seq[i + 2:i + 2 + AH])
            kp_before = stream.n_tracked
            be.drain(); torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            t0 = time.perf_counter()
            for i in range(w1, w1 + n1):
                stream.step(seq[i], seq[i + 1], seq[i + 2:i + 2 + AH])
            be.drain(); torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            dt = max_over_ranks(time.perf_counter() - t0)
            return be, stream, c3, dt, stream.n_tracked - kp_before

        def live_step(fast, lookahead):
            """ONE stream through slam_frontend_step: one C call per frame (u8 frame from host memory -> upload, build graph, matching passes, key-frame work,
            list length), keypoint list resident in HBM; lookahead: the call builds the frame it is given while it matches the one before
            (front_end.jl:58-113, :454-470; mapper.jl:51-66)"""
            u8 = lambda im: np.ascontiguousarray(np.round(np.clip(im, 0, 1) * 255).astype(np.uint8).T)
            L8 = [torch.from_numpy(u8(x)).pin_memory() for x in left]; R8 = [torch.from_numpy(u8(x)).pin_memory() for x in right]      # frames in page-locked host memory (a capture buffer registered once): copied from where they lie
            fe = slam.FrontEnd((H, W), params, extractor, fast=fast, lookahead=lookahead, right_target_only=RIGHT_TARGET_ONLY, device=local_rank)
            camt = tuple(syn.KITTI_CAM)
            T21 = np.eye(4); T21[0, 3] = -0.54
            tri = slam.FrontEnd.tri_params(camt, camt, T21, np.eye(4))
            sps = slam.stream_params(1, cam=camt, shift_yx=(0.0, -disparity))
            g = torch.Generator(device=dev); g.manual_seed(77 + rank)
            culls = [(torch.rand(fe.cap, device=dev, generator=g) < CULL_FRACTION).to(torch.uint8) for _ in range(8)]
            torch.cuda.synchronize()
            rngl = np.random.default_rng(5 + rank)
            fl = np.array(flows)
            total = w1 + n1 + 2
            # the per-frame arguments are INPUT (motion-model prior ~0.5 px off): prepared before the timed region
            pr = [slam.stream_params(1, cam=camt, shift_yx=(fl[seq[t]] - fl[seq[t - 1]] + rngl.normal(0, 0.5, 2)) if t > 0 else (0.0, 0.0)) for t in range(total)]
            def call(t):
                due = t - 1 if lookahead else t
                kfd = due >= 0 and due % KF_EVERY == 0
                return fe.step_ptr(L8[seq[t]].data_ptr(), R8[seq[t]].data_ptr() if t % KF_EVERY == 0 else 0, pr[max(due, 0)].ctypes.data, 2, sps.ctypes.data, 2, tri.ctypes.data,
                                   culls[(due // KF_EVERY) % 8].data_ptr() if kfd and due > 0 else None)      # raw addresses, as a C / Julia host passes them
            tracked = 0
            for t in range(w1):
                call(t)
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            t0 = time.perf_counter()
            for t in range(w1, w1 + n1):
                fr, cnt = call(t)
                if fr >= 0 and fr % KF_EVERY != 0:
                    tracked += cnt
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            dt = max_over_ranks(time.perf_counter() - t0)
            kp = fe.keypoints()
            fe.close()
            return world * n1 / dt, tracked / max(n1 - n1 // KF_EVERY, 1), len(kp["yx"])

    if "single" in legs:
        # ---- the same workload as ONE stream (latency view): 3 contexts, pipelined next-frame pyramid ----
        # builds in flight ahead of the tracking: 1 = the next frame only (rounds 1-2), 3 .. 5 = that many unforked builds (SLAM_PYR_CHAIN) on as
        # many streams, the key-frame's right pyramid requested one frame early on the stream that has just gone idle
        deep = {}
        for ah in (4, 5, 6):                                    # (which depth wins depends on how the runtime maps the streams onto its four hardware queues)
            be_, _, c3_, dt_, _ = one_stream(False, ahead=ah)
            deep[ah] = world * n1 / dt_
            be_.close()
            for c in c3_:
                c.close()
        # the next key-frame period (5 left frames + the key-frame's right frame) as ONE batched build: GpuPeriodBackend
        be_, st_, c3_, dt_, ntr_ = one_stream(False, period=True)
        period_rate, period_tracked = world * n1 / dt_, ntr_ / max(n1, 1)
        period_kp = (st_.kp.copy(), st_.is3d.copy())              # the list after the timed frames: compared with the single-image builds' below
        be_.close()
        for c in c3_:
            c.close()
        be, stream, c3, dt, n_tracked_timed = one_stream(False)
        period_same = bool(np.array_equal(period_kp[0], stream.kp) and np.array_equal(period_kp[1], stream.is3d))
        if not period_same:
            fails.append("single stream: the keypoint list after the timed frames differs between the batched-period builds and the single-image builds")
        # per-kernel device time: a second pass over the same stream with hipEvent spans on
        # the library stream.  Spans force the direct-launch path (the timed region above
        # replays the pyramid build as one hipGraph, which events cannot look inside).
        prof_steps = min(n1, 100)
        be.pipelined = False
        for c in c3:
            c.prof_enable(True); c.prof_reset()
        base = w1 + n1
        for i in range(base, base + prof_steps):
            stream.step(seq[i], seq[i + 1], seq[i + 2:i + 2 + AH])
        pyr_ms, pyr_n = [a + b for a, b in zip(c3[1].prof_get("pyr_update"), c3[2].prof_get("pyr_update"))]
        rows_ms, rows_n = [a + b for a, b in zip(c3[1].prof_get("k_iir_rows"), c3[2].prof_get("k_iir_rows"))]
        fb_ms, fb_n = c3[0].prof_get("fb_track")
        det_ms, det_n = c3[0].prof_get("detect")
        for c in c3:
            c.prof_enable(False)
        best_ah = max(deep, key=deep.get)
        best_rate = max(deep[best_ah], world * n1 / dt, period_rate)
        single = {"value": best_rate, "unit": "frames/sec", "steps": n1, "ms_per_frame": 1e3 * world / best_rate, "streams_per_gpu": 1,
                  "builds_in_flight": "key-frame period as one batch" if period_rate >= best_rate else (best_ah if deep[best_ah] > world * n1 / dt else 1),
                  "by_builds_in_flight": {"1": world * n1 / dt, **{str(k): v for k, v in deep.items()}, "period_batch": period_rate},
                  "tracked_kpts_per_frame": round(n_tracked_timed / max(n1, 1), 1), "tracked_kpts_per_frame_period_batch": round(period_tracked, 1),
                  "period_batch_keypoint_list_identical_to_single_image_builds": period_same,
                  "note": "the same workload as ONE stream per GPU through the single-image entry points, host keypoint lists, every call synchronous as in "
                          "the reference's front-end task; `value` = throughput of one recorded sequence with the left pyramids of the next frames built "
                          "ahead on their own streams (builds_in_flight; by_builds_in_flight[\"1\"] = next frame only, the rounds 1-2 figure; "
                          "\"period_batch\" = the next key-frame period's five left frames + its right frame built by ONE batched launch set, "
                          "slam_pyr_update_batch_dev: same planes bit for bit, the chain-bound single-image kernels stop leaving the GPU idle); "
                          "a frame's own latency is build + track, see device_ms_per_frame"}
        if pyr_n:
            pyr_bytes = pyramid_bytes(H, W, levels)
            rows_bytes = iir_rows_bytes(H, W, levels) / (levels + 1)   # per launch (4 launches / pyramid)
            a = rows_bytes / (rows_ms / rows_n * 1e-3) / 1e9
            single["roofline"] = {"bound": "hbm", "kernel": "k_iir_rows, one image per launch (bound by the dependent f64 chain of the recurrence, not by HBM)",
                                  "achieved": a, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": a / HBM_PEAK_GBS, "traffic": None,
                                  "avg_launch_us": rows_ms / rows_n * 1e3, "algorithmic_bytes_per_launch": rows_bytes,
                                  "stage": {"name": "pyramid update (all kernels of one image)", "algorithmic_bytes": pyr_bytes,
                                            "avg_us": pyr_ms / pyr_n * 1e3, "achieved": pyr_bytes / (pyr_ms / pyr_n * 1e-3) / 1e9,
                                            "frac": pyr_bytes / (pyr_ms / pyr_n * 1e-3) / 1e9 / HBM_PEAK_GBS}}
            single["device_ms_per_frame"] = {"pyr_update_serial_launches": pyr_ms / prof_steps, "fb_track": fb_ms / prof_steps, "detect": det_ms / prof_steps,
                                             "spans_over_steps": prof_steps, "launches": {"pyr_update": pyr_n, "fb_track": fb_n, "detect": det_n}}
        # the live stream as ONE C call per frame (slam_frontend_step, keypoint list in HBM): no Python between the enqueues of a frame
        try:
            v1, trk1, _ = live_step(False, True)
            v0, _, _ = live_step(False, False)
            single["by_builds_in_flight"]["1_python_protocol"] = single["by_builds_in_flight"]["1"]
            single["by_builds_in_flight"]["1"] = v1
            single["live_step"] = {"value": v1, "no_lookahead": v0, "tracked_kpts_per_frame": round(trk1, 1), "unit": "frames/sec",
                                   "what": "slam_frontend_step: one call per frame, frame bytes from host memory, list in HBM; value = the call builds the frame it is given "
                                           "while matching the one before (next frame only); no_lookahead = build + match of the same frame inside the call"}
        except Exception as ex:                                   # noqa: BLE001
            single["live_step"] = {"error": repr(ex)[:300]}
        out["single_stream"] = single
        be.close()
        for c in c3:
            c.close()
        leg_done("single_stream")

    # ---- tolerance-mode pyramid (mode 3: parallel recurrences, planes within 1e-11 rel.), single stream (batches of >= 4 images take
    #      the bit-exact kernels in this mode too) ----
    if "tolerance" in legs:
        be, stream, c3, dtf, _ = one_stream(True, ahead=5)
        out["tolerance_mode"] = {"pyramid": "slam_pyr_update mode 3 (parallel recurrences; planes <= 1e-11 relative, tracked positions <= 1e-7 px vs "
                                            "the bit-exact mode: tests/test_gpu_pyramid.py::test_fast_mode_within_tolerance)",
                                 "single_stream": {"value": world * n1 / dtf, "unit": "frames/sec", "ms_per_frame": dtf / n1 * 1e3, "builds_in_flight": 5}}
        be.close()
        for c in c3:
            c.close()
        be, stream, c3, dtl, _ = one_stream(True)                 # live: the next frame only
        out["tolerance_mode"]["single_stream_live"] = {"value": world * n1 / dtl, "unit": "frames/sec", "ms_per_frame": dtl / n1 * 1e3, "builds_in_flight": 1}
        be.close()
        for c in c3:
            c.close()
        try:
            v1, trk1, _ = live_step(True, True)
            v0, _, _ = live_step(True, False)
            out["tolerance_mode"]["single_stream_live_python_protocol"] = out["tolerance_mode"]["single_stream_live"]
            out["tolerance_mode"]["single_stream_live"] = {"value": v1, "no_lookahead": v0, "unit": "frames/sec", "ms_per_frame": 1e3 * world / v1, "builds_in_flight": 1,
                                                           "tracked_kpts_per_frame": round(trk1, 1), "what": "slam_frontend_step (one C call per frame), tolerance-mode pyramids"}
        except Exception as ex:                                   # noqa: BLE001
            out["tolerance_mode"]["single_stream_live_step_error"] = repr(ex)[:300]
        leg_done("tolerance_mode")

    # ---- headline: S lock-stepped streams per GPU, keypoints resident in HBM, bit-exact planes; frames arrive in host memory as the
    #      decoder's 8-bit images ----
    head = None
    tol_snapshot = None
    dump = args.dump_outputs is not None and rank == 0
    if "headline" in legs:
        # the snapshot (lists + planes of two streams, read after the timed loop) feeds the oracle checks of --full and --dump-outputs
        head = run_lockstep_kpset(slam, torch, local_rank, wl, args.steps, args.warmup, world, dist, dev, "host_u8",
                                  snapshot=[0, S - 1] if full or dump else None, lists=dump)
        leg_done("headline")
        if dump:
            dump_outputs(args.dump_outputs, head)
            del head["lists"]
        if world > 1:
            # every rank's own frame rate over its own clock (`value` = all frames over the SLOWEST rank's time, as the contract asks)
            per_rank = [None] * world
            dist.all_gather_object(per_rank, float(head["value_this_rank"]))
            out["per_rank_values"] = per_rank
            out["sum_of_rank_values"] = float(sum(per_rank))
            if rank == 0:
                # a later leg that loses a rank takes this process with it before the line is printed: the measured headline is left
                # behind for the launcher (spawn_ranks prints it, marked, and exits non-zero)
                try:
                    with open(os.path.join(ROOT, "bench_headline_partial.json"), "w") as f:
                        json.dump({"metric": out["metric"], "value": head["value"], "unit": "frames/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                                   "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
                                   "per_rank_values": per_rank, "config": {"workload": "KITTI-05-shaped stereo 370x1226 @1000 kpts (BASELINE configs[1])", "streams_per_gpu": S}}, f)
                except OSError:
                    pass
        out.update({
            "value": head["value"], "ms_per_step": head["ms_per_step"],
            "config": {"workload": "KITTI-05-shaped stereo streams 370x1226, 1000 kpts/frame, key-frame every 5th frame: "
                                   "left pyramid update + FB-LK (3-D prior pass + 2-D pass) per frame; "
                                   "detect + right pyramid + stereo FB-LK + stereo triangulation per key-frame (BASELINE configs[1]); "
                                   f"one step = one key-frame period = {KF_EVERY} consecutive frames (the first a key-frame) of each of {S} independent streams "
                                   f"= {S * KF_EVERY} frames; frames START IN PINNED HOST MEMORY as the decoder's "
                                   "8-bit images and are copied to the GPU inside the timed loop (one H2D copy per frame step on the copy stream), "
                                   "converted to Float64 on the device; all arithmetic Float64",
                       "frames_start": "pinned host memory, uint8 (example/kitty/kitty.jl:52-102 decode) -- copied H2D inside the timed region",
                       "streams_per_gpu": S, "frames_per_step": S * KF_EVERY, "key_frames_per_step": S, "frame_steps_timed": head["frame_steps"],
                       "ms_per_frame_of_S_streams": head["ms_per_frame_of_S_streams"], "parallelism": f"replicas x{world}",
                       "hbm_in_use_gb": head.get("hbm_in_use_gb"),
                       "pyramid_mode": "bit-exact (slam_pyr_update mode 1 arithmetic; planes identical to the CPU oracle)",
                       "batching": "the S streams advance in lock-step and share every launch: pyramids live in slam_pyr_create_batch batches "
                                   "(grid.z = stream); the keypoint lists live in HBM (slam_kpset_*): tracking + removal of lost keypoints, culling, "
                                   "key-frame detection + merge, stereo matching and triangulation are enqueue-only calls, the host reads the S list "
                                   "lengths once per frame; 4 HIP streams (tracking/detect; left pyramids; right pyramids; copies), the next frames' copy + "
                                   "pyramid build (one hipGraph replay) overlap the current frame's tracking",
                       "tracked_kpts_per_frame": head["tracked_kpts_per_frame"], "host_wait_ms_per_frame": head["host_wait_ms_per_frame"],
                       "window_size": params.window_size, "pyramid_levels": levels,
                       "cull_fraction_per_keyframe": CULL_FRACTION},
        })
    if "headline" in legs and full:
        # the rooflines: the build's per-kernel spans and the graph replay alone are runs of their own, after the timed loop
        rows_us, serial_us, isolated_us = kernel_spans(slam, torch, local_rank, wl, dev)
        pb = S * pyramid_bytes(H, W, levels)
        build_ms = head["pyramid_build_ms"]["mean"]
        rb_bytes = S * iir_rows_bytes(H, W, levels) / (levels + 1)
        out.update({
            # the dominant stage (>= 60 % of the device time of a step): the LK pyramid update of the S images of a frame step.  algorithmic
            # bytes = SURVEY 8(d): 7 planes x 8 B x sum_l H_l W_l per image; duration = hipEvents around the build on the stream it runs on, in
            # the timed region (one hipGraph replay of the ~20 kernels of the build), tracking kernels running beside it
            "roofline": {"bound": "hbm", "stage": f"LK pyramid update of {S} images (pyramid.jl:81-137 + lucas_kanade.jl:109-138): one hipGraph replay, u8 ingest fused",
                         "isolated_launch_us": isolated_us, "frac_isolated": pb / (isolated_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                         "achieved": pb / (build_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": pb / (build_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "frac_of_achievable": pb / (build_ms * 1e-3) / 1e9 / HBM_ACHIEVABLE_GBS, "achievable_peak": HBM_ACHIEVABLE_GBS,
                         "algorithmic_bytes_per_launch": pb, "avg_launch_us": build_ms * 1e3, "launches_timed": head["pyramid_build_ms"]["n"],
                         "min_launch_us": head["pyramid_build_ms"]["min"] * 1e3, "serial_launches_us": serial_us,
                         "traffic": None,
                         "note": "frac / avg_launch_us: hipEvents around every build of the timed region on the pyramid stream -- the tracking kernels of the "
                                 "previous frame run beside the build for its whole duration (own hardware queue), so the duration contains their share of the "
                                 "GPU; frac_isolated / isolated_launch_us: the same graph replay alone on the GPU, back to back",
                         "kernel_local": {"name": "k_iir_rows_ck (dim-2 IIR pass, largest kernel of the build); bytes = 1R + 1W of every plane it filters -- "
                                                  "a kernel-local figure, NOT SURVEY 8d's stage bytes",
                                          "avg_launch_us": rows_us, "bytes_per_launch": rb_bytes,
                                          "achieved": rb_bytes / (rows_us * 1e-6) / 1e9, "frac": rb_bytes / (rows_us * 1e-6) / 1e9 / HBM_PEAK_GBS}},
        })
        lists = [sn["list"]["is_3d"] for sn in head.get("snapshot", {}).values()]
        frac3d = float(np.mean(np.concatenate(lists))) if lists and sum(len(x) for x in lists) else 0.8
        out["roofline"]["frame"], out["roofline"]["lk"] = frame_and_lk_rooflines(wl, head, frac3d)
        pmc = newest_pmc(S)
        if pmc is not None:
            j = json.load(open(pmc))
            out["roofline"]["traffic"] = j["summary"]["all_pyramid_kernels_bytes_per_batch_build"]
            out["roofline"]["traffic_over_algorithmic"] = j["summary"]["all_pyramid_kernels_bytes_per_batch_build"] / pb
            out["roofline"]["traffic_source"] = (f"profiles/{os.path.basename(pmc)} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, FETCH x2 per "
                                                 f"MI355X_MICROARCH.md, WRITE exact), all kernels of one {S}-image build; collected at commit {j.get('commit', 'unrecorded')}")

    # Everything behind the headline is guarded as a whole: an exception in a later leg (the rare runtime error of DESIGN 6 item 6 surfaced in a
    # checker leg once in 17 full runs) is recorded on the line -- `leg_error` -- and the process exits non-zero AFTER printing the headline it has
    # measured; nothing is retried.  (At N > 1 a rank that fails alone leaves its peers in their next collective: the launcher's deadline ends the job.)
    try:
        # ---- the headline loop on TOLERANCE-MODE pyramids (slam_pyr_update_batch mode 3: k_cols_fused<TOL> + k_rows_tol, planes <= 1e-11 relative
        #      to the exact build, tracked positions <= 1e-6 px: tests/test_gpu_tol_batch.py); keypoint indices still come from detect on the raw frame ----
        if "tolbatch" in legs:
            wt = dict(wl); wt["tolerance"] = True
            tb = run_lockstep_kpset(slam, torch, local_rank, wt, max(8, args.steps // 2), 2, world, dist, dev, "host_u8",
                                    snapshot=[0, S // 2, S - 1] if (rank == 0 and world == 1 and "cpu" in legs) else None)
            leg_done("tolbatch")
            tol_snapshot = tb.pop("snapshot", None)                  # checked against the oracle in the cpu leg: tolerance_mode.parity_ok
            _, tserial_us, tiso_us = kernel_spans(slam, torch, local_rank, wt, dev)
            pbt = S * pyramid_bytes(H, W, levels)
            tbm = tb["pyramid_build_ms"]["mean"]
            tnode = out.setdefault("tolerance_mode", {})
            tnode["batch"] = {"value": tb["value"], "unit": "frames/sec", "streams_per_gpu": S, "steps": tb["steps"], "ms_per_step": tb["ms_per_step"],
                              "tracked_kpts_per_frame": tb["tracked_kpts_per_frame"],
                              "lk_match": None if not tb.get("lk_match") else dict(tb["lk_match"], ns_per_point=tb["lk_match"]["mean_ms"] * 1e6 / max(tb["lk_match"]["points_per_launch"], 1),
                                                                                   kernel="k_kpset_match<6, TOL>: contracted arithmetic (positions <= 1e-6 px)"),
                              "pyramid": "slam_pyr_update_batch_u8_dev mode 3: dim-1 stage k_cols_fused<TOL> (product planes leave as suffix sums along y), dim-2 stage + running sum "
                                         "along x + imresize! in ONE kernel k_rows_tol (1 R + 1 W per plane); planes <= 1e-11 relative, positions <= 1e-6 px",
                              "roofline": {"bound": "hbm", "stage": f"LK pyramid update of {S} images, tolerance mode", "algorithmic_bytes_per_launch": pbt,
                                           "avg_launch_us": tbm * 1e3, "achieved": pbt / (tbm * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                           "frac": pbt / (tbm * 1e-3) / 1e9 / HBM_PEAK_GBS, "isolated_launch_us": tiso_us,
                                           "frac_isolated": pbt / (tiso_us * 1e-6) / 1e9 / HBM_PEAK_GBS, "serial_launches_us": tserial_us, "traffic": None}}
            import glob as _g
            c = sorted(_g.glob(os.path.join(ROOT, "profiles", f"r*_pmc_pyramid_tol_batch_s{S}.json")))
            if c:
                j = json.load(open(c[-1]))
                tr = j["summary"]["all_pyramid_kernels_bytes_per_batch_build"]
                tnode["batch"]["roofline"].update({"traffic": tr, "traffic_over_algorithmic": tr / pbt, "traffic_source": f"profiles/{os.path.basename(c[-1])}"})

        # ---- the other ingest configurations of the same loop ----
        if "ingest" in legs:
            out["ingest"] = {}
            if head is not None:
                out["ingest"]["host_u8"] = {"value": head["value"], "ms_per_step": head["ms_per_step"], "steps": head["steps"], "pyramid_build_ms_mean": head["pyramid_build_ms"]["mean"]}
            for ingest in ("dev_f64", "host_f64"):
                v = run_lockstep_kpset(slam, torch, local_rank, wl, max(8, args.steps // 3), 2, world, dist, dev, ingest)
                out["ingest"][ingest] = {"value": v["value"], "ms_per_step": v["ms_per_step"], "steps": v["steps"], "pyramid_build_ms_mean": v["pyramid_build_ms"]["mean"]}
            leg_done("ingest")

        # more streams per GPU share every launch better (the build's per-frame cost falls until the big kernels run whole rounds of
        # workgroups): the same loop at the other batch sizes, short
        if "sweep" in legs and S in (32, 64, 128):
            out["streams_sweep"] = {}
            for S2 in {32: (48, 64), 64: (32, 48), 128: (32, 64, 96)}[S]:
                w2 = dict(wl); w2["S"] = S2
                r2 = run_lockstep_kpset(slam, torch, local_rank, w2, max(8, args.steps // 4), 2, world, dist, dev, "host_u8")
                out["streams_sweep"][str(S2)] = {"value": r2["value"], "unit": "frames/sec", "ms_per_step": r2["ms_per_step"]}
            leg_done("streams_sweep")

        # ---- the round-1 call protocol (keypoint lists on the host, numpy list surgery between the batch seams), frames resident in HBM:
        #      what the device-resident keypoint sets replaced ----
        if "host_protocol" in legs:
            left_dev = [torch.from_numpy(np.ascontiguousarray(im.T)).to(dev) for im in left]
            right_dev = [torch.from_numpy(np.ascontiguousarray(im.T)).to(dev) for im in right]
            torch.cuda.synchronize()
            hp = run_lockstep(slam, torch, local_rank, S, max(40, frame_steps // 4), 10, H, W, left_dev, right_dev, flows, disparity,
                                                               params, extractor, False, world, dist, dev)
            out["host_protocol"] = {"value": hp["value"], "unit": "frames/sec", "ms_per_frame_of_S_streams": hp["ms_per_step_of_S_frames"],
                                    "what": "slam_flow_match_batch_kept / slam_detect_batch with host keypoint lists, frames resident in HBM as Float64 "
                                            "(compare ingest.dev_f64)"}
            del left_dev, right_dev
            leg_done("host_protocol")

        # ---- the other BASELINE shapes through the same loop (their own streams-per-GPU, their own stage roofline) ----
        if "configs" in legs:
            out["configs"] = {}
            import traceback
            for name in ("kitti00_2000", "euroc_mono", "fhd_4000"):
                try:
                    w2 = make_workload(slam, syn, name, seed=rank)
                    mono = not w2["stereo"]
                    r2 = run_lockstep_kpset(slam, torch, local_rank, w2, max(6, args.steps // 4), 2, world, dist, dev, "host_u8", pose=mono)
                    _, serial2, iso2 = kernel_spans(slam, torch, local_rank, w2, dev)
                    pb2 = w2["S"] * pyramid_bytes(w2["H"], w2["W"], w2["levels"])
                    bm = r2["pyramid_build_ms"]["mean"]
                    out["configs"][name] = {
                        "what": w2["what"], "shape": [w2["H"], w2["W"]], "kpts": w2["kpts"], "stereo": w2["stereo"], "streams_per_gpu": w2["S"],
                        "value": r2["value"], "unit": "frames/sec", "steps": r2["steps"], "ms_per_step": r2["ms_per_step"],
                        "ms_per_frame_of_S_streams": r2["ms_per_frame_of_S_streams"], "tracked_kpts_per_frame": r2["tracked_kpts_per_frame"],
                        "pose": r2["pose"],
                        "roofline": {"bound": "hbm", "stage": f"LK pyramid update of {w2['S']} images", "algorithmic_bytes_per_launch": pb2,
                                     "avg_launch_us": bm * 1e3, "achieved": pb2 / (bm * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                     "frac": pb2 / (bm * 1e-3) / 1e9 / HBM_PEAK_GBS, "isolated_launch_us": iso2,
                                     "frac_isolated": pb2 / (iso2 * 1e-6) / 1e9 / HBM_PEAK_GBS, "traffic": None}}
                    if r2["pose"] is not None and not r2["pose"]["pose_ok"]:
                        pose_fails.append(f"configs.{name}: pose check failed ({r2['pose']['max_translation_error_m']:.3f} m, accepted {r2['pose']['accepted_fraction']:.3f})")
                    if "ba" in legs:
                        # the config AS BASELINE NAMES IT: the front-end loop with one local-BA window of the config's size per stream and key-frame period
                        # on the estimator's context + host thread (SlamManager task #3, estimator.jl:78-99, :317-347); a hand-over waits for the previous solve
                        try:
                            worker = BAWorker(slam, syn, local_rank, w2["S"], prio=int(os.environ.get("SLAM_BENCH_BA_PRIO", "1")), window=w2["ba_window"])
                            rb = run_lockstep_kpset(slam, torch, local_rank, w2, max(6, args.steps // 4), 2, world, dist, dev, "host_u8", pose=mono, ba=worker)
                            worker.close()
                            lb = rb["local_ba"]
                            out["configs"][name]["with_ba"] = {"value": rb["value"], "unit": "frames/sec", "fraction_of_front_end_only": rb["value"] / r2["value"],
                                                               "ba_call_ms": lb["mean_call_ms"], "ba_device_ms": lb["device_ms_per_call"], "ba_window": lb["window_name"],
                                                               "windows_per_call": lb["windows_per_call"], "calls": lb["calls"],
                                                               "front_end_waited_ms_per_call": lb["front_end_waited_ms_per_call"], "all_windows_ok": lb["all_windows_ok"],
                                                               "ms_per_step": rb["ms_per_step"], "window": lb["window"]}
                            if not lb["all_windows_ok"]:
                                fails.append(f"configs.{name}.with_ba: a window of the last batch did not solve")
                            del worker, rb
                        except Exception as ex:                               # noqa: BLE001
                            out["configs"][name]["with_ba"] = {"error": repr(ex)[:300]}
                    if "tolbatch" in legs:                                # the same shape on tolerance-mode pyramids (planes <= 1e-11 relative)
                        w2t = dict(w2); w2t["tolerance"] = True
                        r2t = run_lockstep_kpset(slam, torch, local_rank, w2t, max(5, args.steps // 5), 2, world, dist, dev, "host_u8", pose=mono)
                        out["configs"][name]["tolerance_value"] = r2t["value"]
                        out["configs"][name]["tolerance_pyramid_build_ms"] = r2t["pyramid_build_ms"]["mean"]
                        if r2t["pose"] is not None:
                            out["configs"][name]["tolerance_pose"] = r2t["pose"]
                            if not r2t["pose"]["pose_ok"]:
                                pose_fails.append(f"configs.{name} (tolerance mode): pose check failed ({r2t['pose']['max_translation_error_m']:.3f} m)")
                        del w2t
                    del w2
                except Exception as ex:                                   # an optional leg never costs the line: the error goes on the record
                    out["configs"][name] = {"error": repr(ex)[:300] + " | " + " <- ".join(l.strip() for l in traceback.format_exc().splitlines()[-8:-1:2])[:500]}
                    try:
                        torch.cuda.synchronize()
                    except Exception:
                        pass
            leg_done("configs")

        if legs & {"ba", "pose", "cpu"}:
            ctx = slam.Context(local_rank)
        # ---- BA: the windows BASELINE / SURVEY 8d name, single GPU ----
        ba_scenes = None
        if "ba" in legs:
            ba_scenes = ba_windows(syn)
            out["ba"] = {"windows": {}}
            for name, s in ba_scenes.items():
                cache = slam.LocalBACache(s["theta0"].copy(), s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"])
                slam.bundle_adjustment_(cache, s["cam"], ctx=ctx)            # warm-up
                hbw0 = syn.ba_halfband(s)                            # in the caller's pose order
                _, hbw, reordered = slam.ba_plan_order(cache)        # in the order slam_local_ba solves in (loop closures: folded ring)
                best = None
                for _ in range(3):
                    cache = slam.LocalBACache(s["theta0"].copy(), s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"])
                    t0 = time.perf_counter(); slam.bundle_adjustment_(cache, s["cam"], ctx=ctx); wall = time.perf_counter() - t0
                    iters = cache.stats["iters_pass1"] + cache.stats["iters_pass2"]
                    r = {"poses": int(s["P"]), "free_poses": int((np.asarray(s["theta_const"]) == 0).sum()), "observations": int(s["O"]), "points": int(s["M"]),
                         "lm_iterations": iters, "ms_per_iter": cache.stats["device_ms"] / max(iters, 1), "wall_ms_total": wall * 1e3,
                         "ssr_final": cache.stats["ssr_final"], "half_bandwidth": hbw, "half_bandwidth_in_key_frame_order": hbw0, "poses_reordered": reordered,
                         "solver_path": ("banded: k_schur_groups + k_band_solve" + (" on relabelled poses (folded ring, slam_ba_plan_order)" if reordered else ""))
                                        if hbw <= 20 else ("dense: point groups over the whole block triangle (k_schur_groups) + one-workgroup Cholesky from LDS (k_dense_solve)"
                                                           if int((np.asarray(s["theta_const"]) == 0).sum()) <= 30 else "general: pair lists (k_blocks) + tiled Cholesky")}
                    if best is None or r["ms_per_iter"] < best["ms_per_iter"]:
                        best = r
                bytes_iter = 33 * s["O"] + 96 * s["P"] + 48 * s["M"] + 8 * (6 * s["P"]) ** 2
                best["roofline"] = {"bound": "hbm", "algorithmic_bytes_per_iter": int(bytes_iter), "achieved": bytes_iter / (best["ms_per_iter"] * 1e-3) / 1e9,
                                    "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": bytes_iter / (best["ms_per_iter"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                    "note": "latency-bound: a chain of dependent launches and block columns, not bytes"}
                out["ba"]["windows"][name] = best
            # ---- S windows per call (slam_local_ba_batch): what S lock-stepped streams owe per key-frame period ----
            out["ba"]["batch"] = {}
            for bname, Sb in (("P5_free_20_const", S), ("P20", S), ("P50", S), ("P100", min(S, 32))):      # (P100: configs[4] runs 32 streams per GPU)
                mk, _, nbase = BA_WINDOW_SHAPES[bname]
                base = [mk(syn, z) for z in range(nbase)]
                bb = slam.BABatch([slam.LocalBACache(base[z % nbase]["theta0"].copy(), base[z % nbase]["theta_const"], base[z % nbase]["pixels_yx"], base[z % nbase]["pose_ids"],
                                                     base[z % nbase]["point_ids"]) for z in range(Sb)], base[0]["cam"])
                bb.solve(ctx=ctx, reset=True)
                walls = []
                for _ in range(5 if bname in ("P5_free_20_const", "P20") else 3):
                    bb.theta[:] = bb.theta0
                    t0 = time.perf_counter(); bb.solve(ctx=ctx); walls.append(time.perf_counter() - t0)
                one = slam.LocalBACache(base[0]["theta0"].copy(), base[0]["theta_const"], base[0]["pixels_yx"], base[0]["pose_ids"], base[0]["point_ids"])
                slam.bundle_adjustment_(one, base[0]["cam"], ctx=ctx)
                th0, ol0, st0 = bb.window(0)
                same = bool(np.array_equal(ol0, one.outliers) and np.abs(th0 - one.theta).max() <= 1e-6 * max(1.0, np.abs(one.theta).max()))
                if not same:
                    fails.append(f"ba.batch {bname}: window 0 of the batch differs from slam_local_ba on the same arrays")
                # two batches in flight on two contexts through slam_local_ba_batch_begin / _end: plan + staging + upload of one call behind the solve of the other
                dev_ms_blocking = float(bb.stats[0, 6]); its_blocking = float(np.mean(bb.stats[:, 3] + bb.stats[:, 4]))      # (of the blocking calls above: the two-in-flight calls below share the chip)
                piped = None
                if bname in ("P5_free_20_const", "P20"):
                    try:
                        ctx2 = slam.Context(local_rank)
                        b2 = slam.BABatch([slam.LocalBACache(base[z % nbase]["theta0"].copy(), base[z % nbase]["theta_const"], base[z % nbase]["pixels_yx"], base[z % nbase]["pose_ids"],
                                                             base[z % nbase]["point_ids"]) for z in range(Sb)], base[0]["cam"])
                        b2.solve(ctx=ctx2, reset=True)
                        jobs = [(bb, ctx), (b2, ctx2)]
                        ncall = 8
                        t0 = time.perf_counter()
                        jobs[0][0].begin(ctx=jobs[0][1], reset=True)
                        for c_ in range(1, ncall):
                            jobs[c_ % 2][0].begin(ctx=jobs[c_ % 2][1], reset=True)
                            jobs[(c_ - 1) % 2][0].end()
                        jobs[(ncall - 1) % 2][0].end()
                        piped = Sb * ncall / (time.perf_counter() - t0)
                        ok2 = bool((b2.status == 0).all() and np.array_equal(b2.theta, bb.theta))
                        if not ok2:
                            fails.append(f"ba.batch {bname}: the pipelined begin / end calls differ from the blocking call")
                        ctx2.close(); del b2
                    except Exception as ex:                           # noqa: BLE001
                        piped = repr(ex)[:120]
                its = its_blocking
                out["ba"]["batch"][bname] = {"windows": Sb, "observations_per_window": int(base[0]["O"]), "wall_ms_per_call": min(walls) * 1e3, "device_ms_per_call": dev_ms_blocking,
                                             "windows_per_s": Sb / min(walls), "windows_per_s_two_calls_in_flight": piped, "mean_lm_iterations": its, "device_ms_per_iter_of_S_windows": dev_ms_blocking / max(its, 1),
                                             "all_windows_ok": bool((bb.status == 0).all()), "window_0_equals_single_call": same,
                                             "single_window_call_ms": None if bname not in out["ba"]["windows"] else out["ba"]["windows"][bname]["wall_ms_total"],
                                             "what": "slam_local_ba_batch: host set-up of the S windows (threads), one H2D copy, 5 launches per LM iteration for all windows, one D2H copy; "
                                                     "wall clock of the whole call, arrays already concatenated"}
                del bb, base
            p50 = out["ba"]["windows"]["P50"]
            out["ba"].update({"window_kf": 50, "observations": p50["observations"], "points": p50["points"], "lm_iterations": p50["lm_iterations"],
                              "ms_per_iter": p50["ms_per_iter"], "wall_ms_total": p50["wall_ms_total"], "ssr_final": p50["ssr_final"]})
            leg_done("ba")
            # ---- the headline loop with the local BA running inside it: every key-frame step hands the S streams' windows to the estimator
            #      thread (third context), as SlamManager's task #3 does (estimator.jl:78-99) ----
            if head is not None or "headline" not in legs:
                try:
                    worker = BAWorker(slam, syn, local_rank, S, prio=int(os.environ.get("SLAM_BENCH_BA_PRIO", "1")))      # the estimator's context in the HIGH class: its short solve gets its compute units at once and is gone (0.93 -> 0.95-0.97 of the headline, A/B/A/B/A)
                    wb = run_lockstep_kpset(slam, torch, local_rank, wl, max(8, args.steps // 2), 2, world, dist, dev, "host_u8", ba=worker)
                    worker.close()
                    out["frontend_with_ba"] = {"value": wb["value"], "unit": "frames/sec", "ms_per_step": wb["ms_per_step"], "steps": wb["steps"], "local_ba": wb["local_ba"],
                                               "fraction_of_headline": None if head is None else wb["value"] / head["value"],
                                               "what": "the headline loop (bit-exact pyramids) with slam_local_ba_batch of the S streams' windows once per key-frame period on a "
                                                       "third context and host thread; a hand-over waits for the previous solve"}
                    if not wb["local_ba"]["all_windows_ok"]:
                        fails.append("frontend_with_ba: a window of the last batch did not solve")
                except Exception as ex:                               # noqa: BLE001
                    out["frontend_with_ba"] = {"error": repr(ex)[:300]}
                leg_done("frontend_with_ba")
        if "ba_sharded" in legs and world > 1 and os.environ.get("SLAM_BENCH_CHILD") is None:
            # N > 1: the library's own RCCL communicator (slam_comm_*) has never run on real multi-GPU hardware in the build environment.  A
            # collective that does not return cannot be caught as an exception, so every rank runs this leg in a CHILD process (its own
            # process group on another port) under a deadline: a hang costs this object, not the line.
            import subprocess
            env = dict(os.environ, SLAM_BENCH_CHILD="1", MASTER_PORT=str(int(os.environ.get("MASTER_PORT", "29500")) + 17))
            cmd = [sys.executable, os.path.abspath(__file__), "--only", "ba_sharded", "--gpus", str(args.gpus), "--steps", str(args.steps), "--warmup", str(args.warmup)]
            try:
                r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=float(os.environ.get("SLAM_BENCH_SHARDED_TIMEOUT_S", "300")))
                if rank == 0:
                    out["ba_sharded"] = json.loads(r.stdout.strip().split("\n")[-1]).get("ba_sharded", {"error": "the child printed no ba_sharded object", "world_size": world})
            except subprocess.TimeoutExpired:
                out["ba_sharded"] = {"error": "deadline passed: the sharded BA leg did not return (child processes killed)", "world_size": world}
            except Exception as ex:
                out["ba_sharded"] = {"error": repr(ex)[:300], "world_size": world}
        elif "ba_sharded" in legs:
            from slam_jl_amd import sharded_ba
            try:
                # the point-sharded driver (slam_ba_lm_* + RCCL through slam_comm_*): device-paced, one all-reduce + one all-gather per iteration
                sP, sM = (100, 40000) if world > 1 else (50, 10000)
                s2 = syn.ba_scene(P=sP, M=sM, seed=8 if world > 1 else 7)
                sharded_ba.sharded_bundle_adjustment(s2["cam"], s2["theta0"], s2["theta_const"], s2["pixels_yx"], s2["pose_ids"], s2["point_ids"])
                torch.cuda.synchronize()
                if world > 1:
                    dist.barrier()
                t0 = time.perf_counter()
                _, _, st = sharded_ba.sharded_bundle_adjustment(s2["cam"], s2["theta0"], s2["theta_const"], s2["pixels_yx"], s2["pose_ids"], s2["point_ids"])
                torch.cuda.synchronize()
                if world > 1:
                    dist.barrier()
                wall = time.perf_counter() - t0
                _, _, st3 = sharded_ba.sharded_bundle_adjustment(s2["cam"], s2["theta0"], s2["theta_const"], s2["pixels_yx"], s2["pose_ids"], s2["point_ids"], timings={})
                st["collectives_us"] = st3.get("collectives_us")
                out["ba_sharded"] = {"window_kf": sP, "observations": int(s2["O"]), "world_size": world,
                                     "ms_per_iter_wall": (st["lm_wall_ms"] or wall * 1e3) / 15,
                                     "lm_iterations_enqueued": 15, "lm_iterations_effective": st["iters_pass1"] + st["iters_pass2"],
                                     "whole_call_wall_ms": wall * 1e3,
                                     "what": "wall clock of the two device-paced LM passes (enqueue of 5 + 10 iterations: build, RCCL all-reduce of the reduced system, "
                                             "banded solve, all-gather of the trial costs, on-device decision; one host sync per pass) per iteration; the whole call "
                                             "adds host partitioning, shard set-up and the RCCL communicator",
                                     "collectives_us": st.get("collectives_us"),
                                     "worth_sharding": bool(sharded_ba.worth_sharding(sP, s2["O"], world)), "ssr_final": st["ssr_final"],
                                     "model_us_per_iter": sharded_ba.sharding_model(sP, s2["O"], max(world, 2)),
                                     "predicted_crossover_keyframes": {str(n_): sharded_ba.predicted_crossover(n_) for n_ in (2, 4, 8)},          # at 2000 observations per key-frame
                                     "predicted_crossover_keyframes_4000_obs_per_kf": {str(n_): sharded_ba.predicted_crossover(n_, 4000) for n_ in (2, 4, 8)},
                                     "rccl_ranks_seen": world if os.environ.get("SLAM_BENCH_BACKEND", "nccl") == "nccl" else 1,
                                     "rccl_note": "the library's RCCL communicator (slam_comm_*) has only ever run with ONE rank in the build environment (1-GPU boxes); "
                                                  "N > 1 ran over gloo with two processes on one GPU (tests/test_gpu_two_process_shards.py)" if world == 1 or os.environ.get("SLAM_BENCH_BACKEND") == "gloo" else None}
            except Exception as ex:                                   # never lose the line to the optional leg
                out["ba_sharded"] = {"error": repr(ex)[:300], "world_size": world}

        # ---- compute_pose! arithmetic (front_end.jl:164-206): P3P RANSAC (256 triples, 1000 map points) + PnP refinement ----
        # (optional legs behind the headline: an exception in one of them -- a rare capture-state error of the HIP runtime has been
        #  seen once after the RCCL leg -- is recorded in the line instead of losing it)
        def pose_legs():
            ps = syn.p3p_scene(n=1000, seed=3, noise_px=0.4, outlier_frac=0.25, iters=256)
            Kc = ps["K"]; camp = (Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2])
            def pose_once():
                cnt, (KP, inl, err, Rt, bi) = slam.p3p_ransac(ps["pts3d"], ps["px_xy"], ps["pdn"], Kc, threshold=3.0,
                                                                samples=ps["samples"], return_pose=True, ctx=ctx)
                T0 = np.eye(4); T0[:3] = Rt
                slam.pnp_bundle_adjustment(camp, T0, ps["px_xy"][inl][:, ::-1], ps["pts3d"][inl], repr_eps=3.0, ctx=ctx)
                return cnt
            pose_once()
            t0 = time.perf_counter()
            for _ in range(20):
                cnt = pose_once()
            out["pose"] = {"points": 1000, "ransac_triples": 256, "inliers": int(cnt), "ms_per_call": (time.perf_counter() - t0) / 20 * 1e3,
                           "what": "slam_p3p_ransac + slam_pnp_ba, host arrays in and out (wall clock)"}
            # compute_pose_5pt! arithmetic (front_end.jl:305-308): five-point RANSAC, 128 5-tuples, 1000 correspondences
            fs = syn.five_point_scene(n=1000, seed=3, noise_px=0.4, outlier_frac=0.25, iters=128)
            def fp_once():
                return slam.five_point_ransac(fs["px1"], fs["px2"], fs["pd1"], fs["pd2"], fs["K"], fs["K"], max_repr_error=3.0,
                                              samples=fs["samples"], ctx=ctx)[0]
            fp_once()
            t0 = time.perf_counter()
            for _ in range(10):
                cnt5 = fp_once()
            out["pose"]["five_point"] = {"points": 1000, "ransac_tuples": 128, "inliers": int(cnt5),
                                         "ms_per_call": (time.perf_counter() - t0) / 10 * 1e3}
            # the same three seams for S lock-stepped streams: one launch set each (slam_*_batch)
            SB = S
            pss = [syn.p3p_scene(n=1000, seed=40 + z, noise_px=0.4, outlier_frac=0.25, iters=256) for z in range(SB)]
            fss = [syn.five_point_scene(n=1000, seed=40 + z, noise_px=0.4, outlier_frac=0.25, iters=128) for z in range(SB)]
            def pose_batch_once():
                r5 = slam.five_point_ransac_batch([f["px1"] for f in fss], [f["px2"] for f in fss], [f["pd1"] for f in fss], [f["pd2"] for f in fss],
                                                  Kc, Kc, max_repr_error=3.0, samples=[f["samples"] for f in fss], ctx=ctx)
                r3 = slam.p3p_ransac_batch([q["pts3d"] for q in pss], [q["px_xy"] for q in pss], [q["pdn"] for q in pss], Kc, threshold=3.0,
                                           samples=[q["samples"] for q in pss], ctx=ctx)
                poses, pix, pts = [], [], []
                for q, r in zip(pss, r3):
                    T0 = np.eye(4); T0[:3] = r[1][3]
                    poses.append(T0); pix.append(q["px_xy"][r[1][1]][:, ::-1]); pts.append(q["pts3d"][r[1][1]])
                slam.pnp_bundle_adjustment_batch(camp, poses, pix, pts, repr_eps=3.0, ctx=ctx)
                return sum(r[0] for r in r5)
            pose_batch_once()
            t0 = time.perf_counter()
            for _ in range(5):
                pose_batch_once()
            out["pose"]["batch"] = {"streams": SB, "ms_per_step": (time.perf_counter() - t0) / 5 * 1e3,
                                    "what": "five-point RANSAC + P3P RANSAC + PnP refinement for the S streams (3 launch sets), host lists in and out"}
            # compute_pose! on device-resident lists (slam_kpset_compute_pose): the 3-D keypoints never visit the host.  A second set
            # holds the S synthetic scenes (1000 map points each, 25 % gross outliers: they leave the lists in the first call, as
            # in the reference; the timed calls see the 750 consistent points per stream)
            kspose = slam.KeypointSet(SB, 1024, ctx=ctx)
            for z, q in enumerate(pss):
                kspose.upload(z, q["px_xy"][:, ::-1], np.ones(len(q["pts3d"]), bool), q["pts3d"])
                # the previous key-frame sits at the world origin: its observation of every map point (compute_pose_5pt! pairs it with
                # the current pixel; the scene's camera pose is the key-frame -> frame motion)
                Xw = q["pts3d"]
                kf_px = np.stack([camp[1] * Xw[:, 1] / Xw[:, 2] + camp[3], camp[0] * Xw[:, 0] / Xw[:, 2] + camp[2]], axis=1)      # (y, x)
                kspose.upload_keyframe(z, kf_px, Xw[:, 2] > 0.1)
            sp_pose = slam.stream_params(SB, Tcw=np.eye(4), cam=camp)                 # R_compensation = I (no motion-model rotation)
            pose_seed = [0]
            def pose5_kpset_once():
                pose_seed[0] += 1
                return kspose.compute_pose_5pt(sp_pose, min_parallax=5.0, max_repr_error=3.0, iters=128, seed=1000 + pose_seed[0], ctx=ctx)
            def pose_kpset_once():
                pose_seed[0] += 1
                return kspose.compute_pose(sp_pose, threshold=3.0, iters=256, seed=pose_seed[0], ctx=ctx)
            def pose_frontend_once():                                 # front_end.jl:103-113: the epipolar filter, then compute_pose!
                pose5_kpset_once()
                return pose_kpset_once()
            _, s50, n50, par0, c50 = pose5_kpset_once()
            t0 = time.perf_counter()
            for _ in range(10):
                _, s51, n51, par1, c51 = pose5_kpset_once()
            out["pose"]["kpset_5pt"] = {"streams": SB, "ms_per_step": (time.perf_counter() - t0) / 10 * 1e3, "accepted": int(s51.sum()),
                                        "pairs_per_stream": float(c51.mean()), "inliers_first_call": float(n50.mean()), "avg_parallax_px": float(par1.mean()),
                                        "what": "slam_kpset_compute_pose_5pt: pairs with the key-frame observation, parallax, five-point RANSAC (128 tuples), "
                                                "outlier removal for the S streams on device-resident lists"}
            _, st0, ni0, cn0 = pose_kpset_once()
            t0 = time.perf_counter()
            for _ in range(10):
                _, st1, ni1, cn1 = pose_kpset_once()
            out["pose"]["kpset"] = {"streams": SB, "ms_per_step": (time.perf_counter() - t0) / 10 * 1e3, "accepted": int(st1.sum()),
                                    "points_per_stream": float(cn1.mean()), "inliers_first_call": float(ni0.mean()),
                                    "what": "slam_kpset_compute_pose: P3P RANSAC (256 triples) + PnP refinement + outlier removal for the S streams on "
                                            "device-resident lists; one device -> host copy (poses, status, list lengths)"}
            # the tracked workload as the reference's full per-frame front-end on the tracked lists themselves
            wp = run_lockstep_kpset(slam, torch, local_rank, wl, max(8, args.steps // 3), 2, world, dist, dev, "host_u8", pose=True)
            if not wp["pose"]["pose_ok"]:
                pose_fails.append(f"pose.frontend_with_pose: pose check failed ({wp['pose']['max_translation_error_m']:.3f} m, accepted {wp['pose']['accepted_fraction']:.3f})")
            out["pose"]["frontend_with_pose"] = {"value": wp["value"], "unit": "frames/sec", "ms_per_step": wp["ms_per_step"],
                                                 "tracked_kpts_per_frame": wp["tracked_kpts_per_frame"], **wp["pose"],
                                                 "what": "the headline workload as the reference's full per-frame front-end on the tracked lists themselves "
                                                         "(front_end.jl:60-113): tracking with the priors of the predicted pose, slam_kpset_compute_pose_5pt, "
                                                         "slam_kpset_compute_pose every frame, key-frames with slam_kpset_keyframe and triangulation under the "
                                                         "estimated pose; the streams are a rigid scene, the recovered translation is checked against the frames' offsets"}
            wp = run_lockstep_kpset(slam, torch, local_rank, wl, max(4, args.steps // 4), 2, world, dist, dev, "host_u8", hook=pose_batch_once)
            out["pose"]["frontend_with_host_pose_seams"] = {"value": wp["value"], "unit": "frames/sec", "ms_per_step": wp["ms_per_step"],
                                                            "what": "headline workload + slam_five_point_ransac_batch + slam_p3p_ransac_batch + slam_pnp_ba_batch "
                                                                    "every frame (host lists in and out: the round-1 configuration of this figure)"}
            kspose.close()
        if "pose" in legs:
            try:
                pose_legs()
            except Exception as ex:
                out.setdefault("pose", {})["error"] = repr(ex)[:300]
                try:
                    torch.cuda.synchronize()
                except Exception:
                    pass

        # ---- CPU baseline: the oracle on a bounded sample of the same workload (rank 0, N = 1 only); the oracle is also the CHECKER of
        #      the measured GPU paths here: planes of the timed run, a replayed key-frame cycle, every BA window ----
        if rank == 0 and world == 1 and "cpu" in legs:
            from oracle import oracle as orc
            cpu_flags = orc.use_native() or "-O2 -ffp-contract=off"       # -O3 -march=native, compiled on this host
            threads = max(1, min(4, os.cpu_count() or 1))                 # the reference recommends -t4 (docs/src/index.md:60-64)
            cbe = CpuBackend(orc, left, right, params, extractor, threads)
            cs = Stream(cbe, flows, disparity, seed=0)
            cseq = frame_sequence(600)
            cbe.prime(cseq[0])
            n_cpu = 0; t0 = time.perf_counter()
            while n_cpu < 600 and (time.perf_counter() - t0 < 12 or n_cpu < 6):      # ~12 s of CPU work
                cs.step(cseq[n_cpu], cseq[n_cpu + 1], ()); n_cpu += 1
            cdt = time.perf_counter() - t0
            out["cpu_baseline"] = {"value": n_cpu / cdt, "unit": "frames/sec", "cores": threads, "kind": "port",
                                   "sample": f"first {n_cpu} frames of the same stream (incl. {1 + (n_cpu - 1) // KF_EVERY} key-frames) through the C oracle "
                                             f"({cpu_flags}; LK loop OpenMP x{threads}, pyramid/detect single-threaded like the reference); "
                                             f"host has {os.cpu_count()} cores"}
            # -- parity of the front-end the headline measured: (1) the planes the TIMED run left behind, (2) a replayed run of the same
            #    loop (same S, same u8 ingest path, two key-frames) whose keypoint lists the oracle reproduces
            if head is not None:
                par = {"ok": True}
                u8f = lambda im: np.asfortranarray(np.round(im * 255).astype(np.uint8).astype(np.float64) / 255.0)
                n_eq = 0
                for s_, sn in head["snapshot"].items():
                    ref = orc.pyr_build(u8f(left[sn["frame_id"]]), levels, 1.0, 1)
                    for (nm, l), a in sn["planes"].items():
                        eq = bool(np.array_equal(a, ref.plane(nm, l))); n_eq += eq
                        if not eq:
                            par["ok"] = False; fails.append(f"headline planes: stream {s_} {nm} level {l} differ from the oracle")
                par["planes_after_timed_run"] = {"streams": sorted(head["snapshot"]), "planes_compared": 6 * (levels + 1) * len(head["snapshot"]),
                                                 "bit_equal": n_eq, "what": "all planes of the last left pyramids of the timed run vs orc.pyr_build of the same 8-bit frame"}
                rec = {"frame_steps": 7, "steps": []}
                rr = run_lockstep_kpset(slam, torch, local_rank, wl, 0, 0, world, dist, dev, "host_u8", record=rec, snapshot=[0, S - 1])
                worst = 0.0; lists_ok = True
                for s_, sn in rr["snapshot"].items():
                    kp_ref, is3_ref = replay_stream_on_oracle(orc, slam, wl, rec, rr, s_, threads)
                    got = sn["list"]
                    same = len(got["yx"]) == len(kp_ref) and bool(np.array_equal(got["is_3d"], is3_ref))
                    if same and len(kp_ref):
                        worst = max(worst, float(np.abs(got["yx"] - kp_ref).max()))
                    lists_ok &= same
                lists_ok &= worst <= 1e-6
                if not lists_ok:
                    par["ok"] = False; fails.append(f"replayed key-frame cycle: keypoint lists differ from the oracle (max |dpx| {worst})")
                par["replayed_frames"] = {"frames": 7, "key_frames": 2, "streams_per_gpu": S, "streams_checked": sorted(rr["snapshot"]),
                                          "list_lengths_and_3d_flags_equal": bool(lists_ok), "max_abs_position_diff_px": worst,
                                          "keypoints_per_checked_stream": [int(len(sn["list"]["yx"])) for sn in rr["snapshot"].values()],
                                          "what": "the headline loop from empty lists for 7 frames (detect, stereo match, triangulate, 5 temporal matches, cull, detect ...) "
                                                  "with recorded priors / cull flags, replayed per stream through orc.pyr_build / optical_flow_matching / detect / triangulate"}
                out["parity_vs_oracle"] = par
            if head is not None and "tolbatch" in legs:
                # the tolerance twin of replayed_frames: the same recorded 7-frame loop on tolerance-mode pyramids + the contracted tracking kernel, against the
                # oracle's EXACT replay -- keypoints matched by id: positions <= 1e-6 px, fates (tracked / lost / detected) equal for >= 99.5 % of the keypoints
                try:
                    wlt = dict(wl); wlt["tolerance"] = True
                    rec_t = {"frame_steps": 7, "steps": []}
                    rrt = run_lockstep_kpset(slam, torch, local_rank, wlt, 0, 0, world, dist, dev, "host_u8", record=rec_t, snapshot=[0, S - 1])
                    worst_p, n_common, n_union = 0.0, 0, 0
                    for s_, sn in rrt["snapshot"].items():
                        kp_ref, is3_ref, ids_ref = replay_stream_on_oracle(orc, slam, wl, rec_t, rrt, s_, threads, with_ids=True)
                        got = sn["list"]
                        gid = {int(k): n_ for n_, k in enumerate(got["ids"])}; rid = {int(k): n_ for n_, k in enumerate(ids_ref)}
                        common = sorted(set(gid) & set(rid))
                        n_common += len(common); n_union += len(set(gid) | set(rid))
                        if common:
                            a_ = got["yx"][[gid[k] for k in common]]; b_ = kp_ref[[rid[k] for k in common]]
                            same_pt = np.abs(a_ - b_).max(axis=1) <= 0.5          # an id names the same keypoint in both runs unless an earlier fate flip shifted the detections
                            n_common -= int((~same_pt).sum())
                            if same_pt.any():
                                worst_p = max(worst_p, float(np.abs(a_[same_pt] - b_[same_pt]).max()))
                    flips = 1.0 - n_common / max(n_union, 1)
                    ok_t = bool(worst_p <= 1e-6 and flips <= 0.005)
                    out.setdefault("tolerance_mode", {})["replayed_frames"] = {"frames": 7, "key_frames": 2, "streams_checked": sorted(rrt["snapshot"]), "max_abs_position_diff_px": worst_p,
                                                                               "fate_flip_fraction": flips, "keypoints_compared": n_common, "ok": ok_t,
                                                                               "what": "the headline loop on tolerance-mode pyramids (mode 3 batches + the contracted tracking kernel) for 7 frames from "
                                                                                       "empty lists vs the oracle's exact replay with the same recorded priors / cull flags; keypoints matched by id"}
                    if not ok_t:
                        fails.append(f"tolerance-mode replay: max |dpx| {worst_p}, fate flips {flips:.4f}")
                except Exception as ex:                               # noqa: BLE001
                    out.setdefault("tolerance_mode", {})["replayed_frames"] = {"error": repr(ex)[:300]}
            if tol_snapshot:
                # the planes the TIMED tolerance-mode run left behind (S streams, default kernel-selection thresholds) against the oracle's exact build
                u8f = lambda im: np.asfortranarray(np.round(im * 255).astype(np.uint8).astype(np.float64) / 255.0)
                worst_t = 0.0
                for s_, sn in tol_snapshot.items():
                    ref = orc.pyr_build(u8f(left[sn["frame_id"]]), levels, 1.0, 1)
                    for (nm, l), a in sn["planes"].items():
                        r_ = ref.plane(nm, l)
                        worst_t = max(worst_t, float(np.abs(a - r_).max() / max(np.abs(r_).max(), 1e-300)))
                tnode = out.setdefault("tolerance_mode", {})
                tnode["parity_ok"] = bool(worst_t <= 1e-11)
                tnode["parity_vs_oracle"] = {"streams": sorted(tol_snapshot), "planes_compared": 6 * (levels + 1) * len(tol_snapshot), "max_rel_err": worst_t, "bar": 1e-11,
                                             "what": "all planes of the last left pyramids of the timed tolerance-mode run vs orc.pyr_build of the same 8-bit frame, "
                                                     "relative to each plane's largest magnitude"}
                if worst_t > 1e-11:
                    fails.append(f"tolerance-mode batch planes: max relative error {worst_t} > 1e-11")
            if ba_scenes is not None:
                # the measured GPU solver against the oracle on every timed window (parity, not timing: 2 + 3 iterations)
                for name, s in ba_scenes.items():
                    t0 = time.perf_counter()
                    _, _, st1 = orc.bundle_adjustment(s["cam"], s["theta0"], s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"], 2, 3, 5.0, solver=1)
                    c1 = (time.perf_counter() - t0) * 1e3 / max(st1["iters_pass1"] + st1["iters_pass2"], 1)
                    chk = slam.LocalBACache(s["theta0"].copy(), s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"])
                    slam.bundle_adjustment_(chk, s["cam"], iterations=3, iters_fast=2, ctx=ctx)
                    rel = abs(chk.stats["ssr_final"] - st1["ssr_final"]) / st1["ssr_final"]
                    okw = bool(rel <= 1e-8 and chk.stats["n_outliers"] == st1["n_outliers"])
                    if not okw:
                        fails.append(f"BA window {name}: GPU vs oracle Schur-LM rel {rel}, outliers {chk.stats['n_outliers']} vs {st1['n_outliers']}")
                    wv = out["ba"]["windows"][name]
                    wv["parity_vs_oracle"] = {"iters": [2, 3], "ssr_final_gpu": chk.stats["ssr_final"], "ssr_final_oracle_schur": st1["ssr_final"],
                                              "rel_diff_schur": rel, "outliers_equal": bool(chk.stats["n_outliers"] == st1["n_outliers"]), "ok": okw}
                    wv["cpu_ms_per_iter_schur"] = c1
                    if name == "P50":
                        # the timed run's result (the reference's 5 + 10 iterations) against the reference-style solver with the same iteration counts
                        t0 = time.perf_counter()
                        _, _, st0 = orc.bundle_adjustment(s["cam"], s["theta0"], s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"], 5, 10, 5.0, solver=0)
                        c0 = (time.perf_counter() - t0) * 1e3 / max(st0["iters_pass1"] + st0["iters_pass2"], 1)
                        rel0 = abs(wv["ssr_final"] - st0["ssr_final"]) / st0["ssr_final"]
                        if rel0 > 1e-3:                                 # the tests' cross-algorithm bar (tests/test_gpu_ba.py)
                            fails.append(f"BA P50: cost vs reference-style LM+LSMR rel {rel0}")
                        wv["parity_vs_oracle"].update({"ssr_final_oracle_lm_lsmr_5_10": st0["ssr_final"], "ssr_final_gpu_5_10": wv["ssr_final"], "rel_diff_lm_lsmr": rel0})
                        out["ba"]["parity_vs_oracle"] = wv["parity_vs_oracle"]
                        out["ba"]["cpu_ms_per_iter_reference_style_lm_lsmr"] = c0
                        out["ba"]["cpu_ms_per_iter_schur"] = c1
                        out["ba"]["cpu_cores"] = 1
            if "pose" in legs:
                ps = syn.p3p_scene(n=1000, seed=3, noise_px=0.4, outlier_frac=0.25, iters=256)
                t0 = time.perf_counter()
                cnt, KP, Rt, inl, err, bi = orc.p3p_ransac(ps["pts3d"], ps["px_xy"], ps["pdn"], ps["K"], 3.0, ps["samples"])
                T0 = np.eye(4); T0[:3] = Rt
                Kc = ps["K"]
                orc.pnp_ba((Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]), T0, ps["px_xy"][inl][:, ::-1], ps["pts3d"][inl], repr_eps=3.0)
                out.setdefault("pose", {})["cpu_ms_per_call"] = (time.perf_counter() - t0) * 1e3
                out["pose"]["cpu_cores"] = 1
                fs = syn.five_point_scene(n=1000, seed=3, noise_px=0.4, outlier_frac=0.25, iters=128)
                t0 = time.perf_counter()
                orc.five_point_ransac(fs["px1"], fs["px2"], fs["pd1"], fs["pd2"], fs["K"], fs["K"], 3.0, fs["samples"])
                out["pose"].setdefault("five_point", {})["cpu_ms_per_call"] = (time.perf_counter() - t0) * 1e3

    except Exception as ex:                                       # noqa: BLE001
        import traceback
        out["leg_error"] = {"after_leg": progress["last_done"], "error": repr(ex)[:300],
                            "where": " <- ".join(l.strip() for l in traceback.format_exc().splitlines()[-8:-1:2])[:400]}
        try:
            torch.cuda.synchronize()
        except Exception:
            pass

    if pose_fails and not out.get("leg_error"):
        out["leg_error"] = {"after_leg": progress["last_done"], "error": "; ".join(pose_fails)[:300], "where": "pose check of a lock-stepped loop (benchlib/lockstep.py: pose_ok)"}
    if head is not None:
        head.pop("snapshot", None)
    if fails:
        out["parity_failures"] = fails
    if rank == 0 and os.environ.get("SLAM_BENCH_CHILD") is not None:
        print(json.dumps(out), flush=True)                        # a child leg's part of the record, parsed by the parent process
    elif rank == 0:
        write_detail(out)
        sys.stdout.flush()
        print(compact_line(out), flush=True)                      # the LAST stdout line, the one the driver parses
    if world > 1:
        dist.destroy_process_group()
    if fails:                                                     # the line is out; the exit status says a checker disagreed
        print("PARITY FAILURES:\n  " + "\n  ".join(fails), file=sys.stderr)
        raise SystemExit(3)
    if out.get("leg_error"):
        print("LEG ERROR: " + json.dumps(out["leg_error"]), file=sys.stderr)
        raise SystemExit(4)


if __name__ == "__main__":
    main()

