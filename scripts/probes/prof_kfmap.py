"""The key-frame map's three calls at the throughput shape, next to the solve they feed, measured in one session: hipEvent spans (the library's
profiling spans kfmap_add / kfmap_gather_plan / kfmap_gather_emit / kfmap_update) for device time, a host clock around the synchronous gather; after warm-up, median of
repeats with the spread.

Shape: S = 128 streams, 370 x 1226 lists of about 1 000 keypoints, cap 1 400, ring R = 32, table of 16 384 points, a key-frame every 5 frames: between
two key-frames a list loses about a fifth of its keypoints and detection fills it up again; the scene is rigid (points 8 .. 40 m in front of a
camera that moves 0.3 m sideways per key-frame, 0.3 px of pixel noise, 2 cm of triangulation noise), so the windows are solvable.  Warm-up runs
8 key-frames (the covisibility map is full: 5 key-frames, older observers outside it); then per repeat one key-frame of all S streams:
  (a) device time of slam_kfmap_add_keyframe;
  (b) device time (plan + emit kernels) and synchronous wall time of slam_kfmap_ba_gather;
  (c) device time of slam_local_ba_batch on the gathered windows (its own figure, stats[6]);
  (d) device time of slam_kfmap_ba_update with the live lists following.
With --filter the sequence runs a second time with map_filtering! behind every update (KeyframeMap.filter at the reference's defaults:
filtering_ratio 0.9, min_cov_score 25, first key-frame 20), and the record is the filter's instead:
  (e) device time of slam_kfmap_filter (span kfmap_filter), with the per-step figures and the key-frames each step removed, and the mean window
      P / M / O of the same steps' gathers with and without the filter -- what the filter is for.

    python scripts/probes/prof_kfmap.py [--streams 128] [--repeats 25] [--out profiles/kfmap_s128.json]
    python scripts/probes/prof_kfmap.py --filter [--out profiles/kfmap_filter_s128.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
H, W, CAP, NKP, RING, MCAP, WARM = 370, 1226, 1400, 1000, 32, 16384, 8


def stat(v):
    v = [float(x) for x in v]
    if not v:
        return None
    return {"median": round(float(np.median(v)), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


class Stream:
    """the scripted list of one stream: ids ascending, world points, 3-D flags"""

    def __init__(self, rng, cam):
        self.rng, self.cam = rng, cam
        self.ids = np.zeros(0, np.int64); self.X = np.zeros((0, 3)); self.f3 = np.zeros(0, bool); self.next = 0

    def project(self, k):
        fx, fy, cx, cy = self.cam
        Xc = self.X - np.array([0.3 * k, 0.0, 0.0])
        return np.stack([fy * Xc[:, 1] / Xc[:, 2] + cy, fx * Xc[:, 0] / Xc[:, 2] + cx], axis=1)

    def keyframe(self, k):
        """-> (Tcw, yx, is_3d, xyz, ids) of key-frame k"""
        rng, (fx, fy, cx, cy) = self.rng, self.cam
        yx = self.project(k)
        keep = (rng.random(len(self.ids)) > 0.2) & (yx[:, 0] > 2) & (yx[:, 0] < H - 2) & (yx[:, 1] > 2) & (yx[:, 1] < W - 2)
        self.ids, self.X, self.f3 = self.ids[keep], self.X[keep], self.f3[keep] | (rng.random(int(keep.sum())) < 0.5)
        n_new = max(NKP + int(rng.integers(-40, 40)) - len(self.ids), 0)
        z = rng.uniform(8.0, 40.0, n_new); py = rng.uniform(3, H - 3, n_new); px = rng.uniform(3, W - 3, n_new)
        Xn = np.stack([(px - cx) / fx * z + 0.3 * k, (py - cy) / fy * z, z], axis=1)
        self.ids = np.concatenate([self.ids, self.next + np.arange(n_new)]); self.next += n_new
        self.X = np.concatenate([self.X, Xn]); self.f3 = np.concatenate([self.f3, rng.random(n_new) < 0.6])
        T = np.eye(4); T[0, 3] = -0.3 * k
        n = len(self.ids)
        return T, self.project(k) + rng.normal(0, 0.3, (n, 2)), self.f3.copy(), self.X + rng.normal(0, 0.02, (n, 3)), self.ids.copy()


def sequence(slam, ctx, cam, S, R, do_filter):
    """WARM + R key-frames of all S streams through the map's calls -> the per-step measurements of the last R"""
    streams = [Stream(np.random.default_rng(100 + s), cam) for s in range(S)]
    ks = slam.KeypointSet(S, CAP)
    km = slam.KeyframeMap(S, CAP, R=RING, mcap=MCAP)
    m = {k: [] for k in ("add", "gather", "plan", "emit", "wall", "solve", "update", "sizes", "filter", "removed", "kfid")}
    ctx.prof_enable(True)
    for k in range(WARM + R):
        Tcw = np.tile(np.eye(4), (S, 1, 1))
        for s, st in enumerate(streams):
            Tcw[s], yx, f3, xyz, ids = st.keyframe(k)
            ks.upload(s, yx, f3, xyz, ids)
        sp = slam.stream_params(S, Tcw=Tcw, cam=cam)
        ks.keyframe()
        ctx.synchronize()
        ctx.prof_reset()
        km.add_keyframe(ks, sp)
        ctx.synchronize()
        wins, status = km.gather(25)
        wall = km.last_gather_ms                                 # the C call alone, without the wrapper's array slicing
        assert not (status == 2).any(), "a window did not fit the probe's capacities"
        if wins:
            slam.bundle_adjustment_batch_([w.cache for w in wins], cam)
            km.update(wins, ks=ks)
        removed = km.filter(0.9, 25) if do_filter else [[]] * S
        ctx.synchronize()
        if k >= WARM:
            m["add"].append(ctx.prof_get("kfmap_add")[0]); m["plan"].append(ctx.prof_get("kfmap_gather_plan")[0]); m["emit"].append(ctx.prof_get("kfmap_gather_emit")[0])
            m["gather"].append(m["plan"][-1] + m["emit"][-1]); m["update"].append(ctx.prof_get("kfmap_update")[0])
            m["wall"].append(wall); m["solve"].append(wins[0].cache.stats["device_ms"])
            m["sizes"].append([np.mean([w.cache.n_poses for w in wins]), np.mean([w.cache.n_points for w in wins]), np.mean([len(w.cache.poses_ids) for w in wins]), len(wins)])
            if do_filter:
                m["filter"].append(ctx.prof_get("kfmap_filter")[0]); m["removed"].append(sum(len(r) for r in removed)); m["kfid"].append(k)
    ctx.prof_enable(False)
    km.close(); ks.close()
    return m


def window_mean(m):
    sz = np.mean(np.array(m["sizes"]), axis=0)
    return float(sz[3]), {"poses": float(sz[0]), "points": float(sz[1]), "observations": float(sz[2])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--filter", action="store_true", help="measure slam_kfmap_filter: the sequence once without and once with the filter behind every update")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import slam_jl_amd as slam
    from slam_jl_amd import synthetic as syn
    S, R = args.streams, args.repeats
    ctx = slam.default_context(0)                                # no device: raises here, nothing is measured
    cam = syn.KITTI_CAM
    m = sequence(slam, ctx, cam, S, R, False)
    n_win, wmean = window_mean(m)
    base = {"lib": os.path.basename(slam.LIB_PATH), "S": S, "cap": CAP, "keypoints_per_stream": NKP, "shape": [H, W], "ring": RING, "table": MCAP, "repeats": R,
            "warmup_keyframes": WARM}
    if args.filter:
        f = sequence(slam, ctx, cam, S, R, True)
        rec = dict(base, filtering_ratio=0.9, min_cov_score=25, first_kfid=20, e_filter_device_ms=stat(f["filter"]),
                   e_filter_device_ms_steps_before_first_kfid=stat([t for t, k in zip(f["filter"], f["kfid"]) if k < 20]),
                   e_filter_device_ms_steps_from_first_kfid=stat([t for t, k in zip(f["filter"], f["kfid"]) if k >= 20]),
                   per_step=[{"keyframe": k, "filter_ms": round(float(t), 5), "removed_all_streams": int(n)} for k, t, n in zip(f["kfid"], f["filter"], f["removed"])],
                   keyframes_removed=int(sum(f["removed"])), window_mean_without_filter=wmean, window_mean_with_filter=window_mean(f)[1],
                   b_gather_plan_kernel_ms_without_filter=stat(m["plan"]), b_gather_plan_kernel_ms_with_filter=stat(f["plan"]),
                   c_local_ba_batch_device_ms_without_filter=stat(m["solve"]), c_local_ba_batch_device_ms_with_filter=stat(f["solve"]))
    else:
        rec = dict(base, windows_per_step=n_win, window_mean=wmean,
                   a_add_keyframe_device_ms=stat(m["add"]), b_gather_device_ms=stat(m["gather"]), b_gather_plan_kernel_ms=stat(m["plan"]), b_gather_emit_kernel_ms=stat(m["emit"]),
                   b_gather_sync_wall_ms=stat(m["wall"]), c_local_ba_batch_device_ms=stat(m["solve"]), d_update_device_ms=stat(m["update"]),
                   map_calls_device_ms_median_sum=round(float(np.median(m["add"]) + np.median(m["gather"]) + np.median(m["update"])), 5))
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f_:
            f_.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
