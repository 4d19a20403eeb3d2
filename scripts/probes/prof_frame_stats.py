"""slam_kpset_frame_stats at the throughput shape, timed with hipEvents (the library's profiling span `kpset_frame_stats`) and a host clock around the
calls that end in a stream wait; after warm-up, median of repeats with the spread.

Shape: S = 128 streams, cap 1400, about 1100 keypoints per stream in a 370 x 1226 image (the headline's lists after a key-frame period), 85 % of
them observed by the previous key-frame, 40 % 3-D, KITTI camera, a 2 degree compensation (none in the stationary case), cell 35.
  (a) device time of k_kpset_frame_stats (flags = 1);
  (b) wall time of the synchronous call (S x 8 doubles come back), next to the wall time of slam_kpset_counts on the same set: the read-back it
      replaces.  Both through ctypes on prepared arrays, alternating.
  (c) the same with every parallax equal (a stationary camera: all terms fall into one bin of every histogram pass, the worst case for the LDS
      atomics), and the enqueue-only form's host time.

    python scripts/probes/prof_frame_stats.py [--streams 128] [--repeats 25] [--out profiles/frame_stats_s128.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
H, W, CELL, CAP, NKP = 370, 1226, 35, 1400, 1100


def stat(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import slam_jl_amd as slam
    from slam_jl_amd import _lib as L, synthetic as syn
    S, R = args.streams, args.repeats
    ctx = slam.default_context(0)                                # no device: raises here, nothing is measured
    rng = np.random.default_rng(5)
    a = np.deg2rad(2.0)
    T = np.tile(np.eye(4), (S, 1, 1)); T[:, 0, 0] = T[:, 2, 2] = np.cos(a); T[:, 0, 2] = np.sin(a); T[:, 2, 0] = -np.sin(a)

    def params(Tc):
        sp = slam.stream_params(S, Tcw=Tc, cam=syn.KITTI_CAM)
        sp[:, :9] = sp[:, :16].reshape(S, 4, 4)[:, :3, :3].reshape(S, 9)        # the seam's dense 3 x 3 (KeypointSet.frame_stats does this per call)
        return np.ascontiguousarray(sp)

    def filled(stationary):
        ks = slam.KeypointSet(S, CAP)
        for s in range(S):
            n = NKP + int(rng.integers(-60, 60))
            kyx = np.stack([rng.uniform(3, H - 3, n), rng.uniform(3, W - 3, n)], axis=1)
            yx = kyx.copy() if stationary else kyx + rng.normal(0, 6.0, (n, 2)) + (2.0, -7.0)
            ks.upload(s, yx, rng.random(n) < 0.4)
            ks.upload_keyframe(s, kyx, rng.random(n) < 0.85)
        return ks

    rec = {"lib": os.path.basename(slam.LIB_PATH), "S": S, "cap": CAP, "keypoints_per_stream": NKP, "shape": [H, W], "cell_size": CELL, "repeats": R, "cases": []}
    for tag, stationary in (("moving camera", False), ("stationary camera (all terms equal)", True)):
        ks = filled(stationary)
        sp = params(np.tile(np.eye(4), (S, 1, 1)) if stationary else T)          # stationary: no rotation either, every term is exactly 0
        out = np.zeros((S, 8)); cnt = np.zeros(S, np.int32)
        sync = lambda: ctx.check(ctx.lib.slam_kpset_frame_stats(ctx.h, ks.h, L.ptr(sp), 1, CELL, H, W, None, L.ptr(out)))
        enq = lambda: ctx.check(ctx.lib.slam_kpset_frame_stats(ctx.h, ks.h, L.ptr(sp), 1, CELL, H, W, None, None))
        counts = lambda: ctx.check(ctx.lib.slam_kpset_counts(ctx.h, ks.h, L.ptr(cnt, L.i32p)))
        for _ in range(5):
            sync(); counts(); enq()
        ctx.synchronize()
        dev, w_sync, w_cnt, w_enq = [], [], [], []
        ctx.prof_enable(True)                                    # device time: the span's events are recorded only here
        for _ in range(R):
            ctx.prof_reset()
            sync()
            dev.append(ctx.prof_get("kpset_frame_stats")[0])
        ctx.prof_enable(False)
        for _ in range(R):                                       # wall times, profiling off
            t0 = time.perf_counter(); sync(); w_sync.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); counts(); w_cnt.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); enq(); w_enq.append((time.perf_counter() - t0) * 1e3)
            ctx.synchronize()
        assert np.array_equal(out[:, 0].astype(np.int32), cnt)
        rec["cases"].append({"case": tag, "n_parallax_mean": float(out[:, 5].mean()), "median_parallax_mean_px": float(out[:, 7].mean()),
                             "a_kernel_ms": stat(dev), "b_sync_call_wall_ms": stat(w_sync), "b_kpset_counts_wall_ms": stat(w_cnt), "c_enqueue_only_host_ms": stat(w_enq)})
        ks.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
