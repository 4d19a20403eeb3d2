"""describe() at the throughput shape, three ways, timed with hipEvents (the library's profiling spans) and a host clock around calls that end in a
stream wait; after warm-up, median of repeats with the spread.

Shape: S = 128 streams of 370 x 1226 u8 frames (a few distinct textures repeated over the streams), extractor 1000 points / radius 17 / cell 35,
BRIEF 256 bits, window 9.  Two workloads: the FIRST key-frame (empty lists, about 1000 keypoints per stream) and a STEADY-STATE key-frame (the
lists after four tracked frames and the 15 % map cull bench.py's headline applies per key-frame; the key-frame refills them).  For each:
  (a) the host-image way: S calls of slam_describe on Float64 host images (upload + two full-frame passes each), wall time;
  (b) slam_describe_batch on the resident pyramids: device time of k_brief_patch (span "describe") and wall time of the call;
  (c) slam_kpset_detect_describe against slam_kpset_detect on identical sets, alternating: the device time the border drop and the describe
      stage add to a key-frame, also as a share of detect_cells' own time.

    python scripts/probes/prof_describe.py [--streams 128] [--repeats 25] [--distinct 4] [--out profiles/describe_s128.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
H, W, CELL, MAXP, RADIUS, NBITS, WINDOW, TRACKED, CULL = 370, 1226, 35, 1000, 17, 256, 9, 4, 0.15


def stat(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import slam_jl_amd as slam
    from slam_jl_amd import _lib as L, synthetic as syn
    S, R = args.streams, max(20, args.repeats)
    ctx = slam.default_context(0)                                # no device: raises here, nothing is measured
    q8 = lambda im: np.asfortranarray(np.round(im * 255).astype(np.uint8))
    tex = [syn.stereo_stream((H, W), TRACKED + 1, seed=60 + d) for d in range(args.distinct)]
    u8 = [[q8(im) for im in t[0]] for t in tex]                  # [distinct][frame]
    step = np.array(tex[0][2][1])
    dev = torch.from_numpy(np.stack([np.stack([np.ascontiguousarray(u8[s % args.distinct][f].T) for s in range(S)]) for f in range(TRACKED + 1)])).cuda()
    torch.cuda.synchronize()
    ptrs = lambda f: [dev[f, s].data_ptr() for s in range(S)]
    grid = (-(-H // CELL), -(-W // CELL))
    ncell = grid[0] * grid[1]
    e = slam.Extractor(MAXP, RADIUS, grid, CELL)
    dcap = ncell * -(-MAXP // ncell)
    cap = MAXP + ncell + 8
    pat = slam.brief_pattern(NBITS, WINDOW)
    words = NBITS // 64
    params = slam.Params(max_nb_keypoints=MAXP)
    batches = [slam.PyramidBatch((H, W), levels=3, S=S) for _ in range(2)]
    desc = torch.zeros((S, dcap, words), dtype=torch.int64, device="cuda")
    info = torch.zeros((S, 2), dtype=torch.int64, device="cuda")
    ksA, ksB = slam.KeypointSet(S, cap), slam.KeypointSet(S, cap)

    def key_frame(tag, batch, frame, state):
        """state[s] = (yx, ids) of stream s before the key-frame"""
        host = [np.asfortranarray(u8[s % args.distinct][frame].astype(np.float64) / 255.0) for s in range(args.distinct)]
        cur = np.concatenate([st[0] for st in state]); sid = np.concatenate([np.full(len(st[0]), s, np.int32) for s, st in enumerate(state)])
        kp, ksid = slam.detect_batch(e, batch, cur, sid)          # what the key-frame detects: the list describe() gets
        off = np.zeros(S + 1, np.int32); off[1:] = np.cumsum(np.bincount(ksid, minlength=S))
        per = [np.ascontiguousarray(kp[off[s]:off[s + 1]]) for s in range(S)]
        bits = np.zeros((len(kp), words), np.uint64); orc_ = np.zeros((len(kp), 2), np.int64); ooff = np.zeros(S + 1, np.int32); n = C.c_int(0)

        hbits = np.zeros_like(bits); hrc = np.zeros_like(orc_)

        def host_way():
            o = 0                                                # survivors of all streams back to back, as the batch form returns them
            for s in range(S):
                ctx.check(ctx.lib.slam_describe(ctx.h, L.ptr(host[s % args.distinct]), H, W, L.ptr(per[s], L.i64p), len(per[s]), L.ptr(pat, L.i32p), NBITS,
                                                float(np.sqrt(2.0)), WINDOW, L.ptr(hbits[o:], L.u64p), L.ptr(hrc[o:], L.i64p), C.byref(n)))
                o += n.value
            return o

        def batch_way():
            ctx.check(ctx.lib.slam_describe_batch(ctx.h, batch.pyramids[0].h, S, L.ptr(kp, L.i64p), L.ptr(off, L.i32p), L.ptr(pat, L.i32p), NBITS,
                                                  float(np.sqrt(2.0)), WINDOW, L.ptr(bits, L.u64p), L.ptr(orc_, L.i64p), L.ptr(ooff, L.i32p)))

        def restore(ks):
            for s, (yx, ids) in enumerate(state):
                ks.upload(s, yx, np.zeros(len(yx), bool), ids=ids)

        for _ in range(2):                                       # warm-up of every shape the timed window uses
            host_way(); batch_way()
            restore(ksA); restore(ksB)
            ksA.detect_describe(e, batch, desc.data_ptr(), info.data_ptr(), dcap, pattern=pat, window=WINDOW); ksB.detect(e, batch)
        ctx.synchronize()
        kept = int(ooff[S])
        assert host_way() == kept and np.array_equal(hbits[:kept], bits[:kept]) and np.array_equal(hrc[:kept], orc_[:kept]), "slam_describe_batch and slam_describe disagree"
        a_wall, b_wall, b_dev, c_dd, c_desc, c_cells, c_det = [], [], [], [], [], [], []
        ctx.prof_enable(True)
        for _ in range(R):
            t0 = time.perf_counter(); host_way(); a_wall.append((time.perf_counter() - t0) * 1e3)
            ctx.prof_reset()
            t0 = time.perf_counter(); batch_way(); b_wall.append((time.perf_counter() - t0) * 1e3)
            b_dev.append(ctx.prof_get("describe")[0])
            restore(ksA); restore(ksB)
            ctx.prof_reset()
            ksA.detect_describe(e, batch, desc.data_ptr(), info.data_ptr(), dcap, pattern=pat, window=WINDOW)
            c_dd.append(ctx.prof_get("detect")[0]); c_desc.append(ctx.prof_get("describe")[0]); c_cells.append(ctx.prof_get("detect_cells")[0])
            ctx.prof_reset()
            ksB.detect(e, batch)
            c_det.append(ctx.prof_get("detect")[0])
        ctx.prof_enable(False)
        added = [x + y - z for x, y, z in zip(c_dd, c_desc, c_det)]
        appended = int(info.cpu().numpy()[:, 1].sum())
        return {"workload": tag, "keypoints_in_lists": int(len(cur)), "detected": int(len(kp)), "described": kept, "appended_by_detect_describe": appended,
                "a_host_image_calls_wall_ms": stat(a_wall), "b_batch_wall_ms": stat(b_wall), "b_batch_kernel_ms": stat(b_dev),
                "b_kernel_ns_per_keypoint": round(1e6 * float(np.median(b_dev)) / max(kept, 1), 3),
                "c_detect_describe_detect_span_ms": stat(c_dd), "c_detect_describe_describe_span_ms": stat(c_desc), "c_detect_cells_ms": stat(c_cells),
                "c_kpset_detect_span_ms": stat(c_det), "c_added_device_ms": stat(added),
                "c_added_share_of_detect_cells": round(float(np.median(added)) / float(np.median(c_cells)), 4)}

    rec = {"lib": os.path.basename(slam.LIB_PATH), "S": S, "shape": [H, W], "n_bits": NBITS, "window": WINDOW, "max_points": MAXP, "repeats": R,
           "distinct_textures": args.distinct, "workloads": []}
    batches[0].update_(ptrs(0), u8=True)
    empty = [(np.zeros((0, 2)), np.zeros(0, np.int64))] * S
    rec["workloads"].append(key_frame("first key-frame", batches[0], 0, empty))
    # steady state: key-frame on frame 0, four tracked frames, then the key-frame that is measured
    ks = slam.KeypointSet(S, cap)
    ks.detect_describe(e, batches[0], desc.data_ptr(), info.data_ptr(), dcap, pattern=pat, window=WINDOW)
    ks.keyframe()
    sp = slam.stream_params(S, cam=syn.KITTI_CAM, shift_yx=np.tile(step, (S, 1)))
    for f in range(1, TRACKED + 1):
        prev, curb = batches[(f - 1) % 2], batches[f % 2]
        curb.update_(ptrs(f), u8=True)
        ks.flow_match(prev, curb, params, sp, prior=2)
    # map culling before the key-frame, as bench.py's headline does it (15 % of every list, flags drawn in HBM): without it the lists stay at
    # max_points over four frames of this smooth synthetic motion and the key-frame detects nothing
    cnt = ks.counts()
    rng = np.random.default_rng(9)
    flags = np.zeros((S, cap), np.uint8)
    for s in range(S):
        flags[s, :cnt[s]] = rng.random(cnt[s]) < CULL
    fdev = torch.from_numpy(flags).cuda(); torch.cuda.synchronize()
    ks.remove(fdev.data_ptr())
    state = []
    for s in range(S):
        g = ks.download(s)
        state.append((g["yx"], g["ids"]))
    rec["workloads"].append(key_frame("steady-state key-frame after %d tracked frames and a %d %% cull" % (TRACKED, round(100 * CULL)), batches[TRACKED % 2], TRACKED, state))
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
