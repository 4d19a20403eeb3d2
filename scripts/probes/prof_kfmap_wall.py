"""Host wall time of the key-frame map's enqueue-only calls at prof_kfmap.py's shape and sequence (S = 128, cap 1 400, R 32, mcap 16 384, 8 warm-up
key-frames): slam_kfmap_add_keyframe, slam_kfmap_ba_update with the lists following, slam_kfmap_filter without its read-back -- each through its Python
wrapper, on an idle stream (a synchronize in front of the clock), median of the repeats with the spread.  What the calls cost the host that enqueues
them: argument checks, staging through the map's pinned block, launches.  (slam_kfmap_merge's wall time is prof_kfmap_merge.py's.)

    python scripts/probes/prof_kfmap_wall.py [--streams 128] [--repeats 25] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prof_kfmap as pk  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import slam_jl_amd as slam
    from slam_jl_amd import synthetic as syn
    S, R = args.streams, args.repeats
    ctx = slam.default_context(0)                                # no device: raises here, nothing is measured
    cam = syn.KITTI_CAM
    streams = [pk.Stream(np.random.default_rng(100 + s), cam) for s in range(S)]
    ks = slam.KeypointSet(S, pk.CAP)
    km = slam.KeyframeMap(S, pk.CAP, R=pk.RING, mcap=pk.MCAP)
    m = {"add": [], "update": [], "filter": []}

    def timed(key, k, call):
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        dt = (time.perf_counter() - t0) * 1e3
        if k >= pk.WARM:
            m[key].append(dt)
    for k in range(pk.WARM + R):
        Tcw = np.tile(np.eye(4), (S, 1, 1))
        for s, st in enumerate(streams):
            Tcw[s], yx, f3, xyz, ids = st.keyframe(k)
            ks.upload(s, yx, f3, xyz, ids)
        sp = slam.stream_params(S, Tcw=Tcw, cam=cam)
        ks.keyframe()
        timed("add", k, lambda: km.add_keyframe(ks, sp))
        wins, status = km.gather(25)
        if wins:
            slam.bundle_adjustment_batch_([w.cache for w in wins], cam)
            timed("update", k, lambda: km.update(wins, ks=ks))
        timed("filter", k, lambda: km.filter(0.9, 25, want_removed=False))
    ctx.synchronize()
    km.close(); ks.close()
    rec = {"lib": os.path.basename(slam.LIB_PATH), "S": S, "cap": pk.CAP, "keypoints_per_stream": pk.NKP, "ring": pk.RING, "table": pk.MCAP, "repeats": R,
           "warmup_keyframes": pk.WARM, "add_keyframe_wall_ms": pk.stat(m["add"]), "update_wall_ms": pk.stat(m["update"]), "filter_enqueue_wall_ms": pk.stat(m["filter"])}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f_:
            f_.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
