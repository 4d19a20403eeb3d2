"""Temporal triangulation of a key-frame step at the throughput shape, the two routes alternating in one session:
  set route   KeypointSet.triangulate_temporal as a host pays for it today: the S x nkf x 4 matrices formed in Python, staged through pinned memory, the
              kernel, the compaction and the blocking wait -- wall time of the call;
  map route   KeyframeMap.triangulate_temporal(ks=ks, want_counts=False) followed by one ctx.synchronize() -- wall time of both; the device times of
              its two kernels (spans kfmap_tri_poses, kfmap_tri_temporal: hipEvents around each launch).

Shape: S = 128 streams, cap 1 400, ring R = 32, table of 16 384 points, lists of about 1 300 keypoints of which about 350 are born 2-D at every
key-frame; those that survive to their second key-frame (about 250-300 per stream) are that step's candidates, afterwards they are 3-D.  Both routes see
the same scripted lists: route A has a KeypointSet of its own whose slots remember the first observation (upload_first) and a ring of NKF = 8 host poses,
route B a KeypointSet and a KeyframeMap.  Which route goes first alternates from step to step.  Warm-up 8 key-frames; medians with the spread (min - max).

    python scripts/probes/prof_kfmap_tri.py [--streams 128] [--repeats 16] [--out profiles/kfmap_tri_s128.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from prof_kfmap import CAP, H, MCAP, RING, W, WARM, stat  # noqa: E402

NKP, DROP, NKF = 1300, 0.27, 8


class MonoStream:
    """the scripted list of one stream: ids ascending, world points; a point is 2-D at its first two key-frames (a candidate at the second), 3-D after"""

    def __init__(self, rng, cam):
        self.rng, self.cam = rng, cam
        self.ids = np.zeros(0, np.int64); self.X = np.zeros((0, 3)); self.age = np.zeros(0, np.int64); self.fyx = np.zeros((0, 2)); self.fkf = np.zeros(0, np.int32)
        self.next = 0

    def project(self, X, k):
        fx, fy, cx, cy = self.cam
        Xc = X - np.array([0.3 * k, 0.0, 0.0])
        return np.stack([fy * Xc[:, 1] / Xc[:, 2] + cy, fx * Xc[:, 0] / Xc[:, 2] + cx], axis=1)

    def keyframe(self, k):
        """-> (Tcw, yx, is_3d, xyz, ids, first yx, first key-frame) of key-frame k"""
        rng, (fx, fy, cx, cy) = self.rng, self.cam
        keep = rng.random(len(self.ids)) > DROP
        self.ids, self.X, self.age, self.fyx, self.fkf = self.ids[keep], self.X[keep], self.age[keep] + 1, self.fyx[keep], self.fkf[keep]
        n_new = max(NKP + int(rng.integers(-40, 40)) - len(self.ids), 0)
        z = rng.uniform(8.0, 40.0, n_new); py = rng.uniform(3, H - 3, n_new); px = rng.uniform(3, W - 3, n_new)
        Xn = np.stack([(px - cx) / fx * z + 0.3 * k, (py - cy) / fy * z, z], axis=1)
        yx_new = self.project(Xn, k) + rng.normal(0, 0.3, (n_new, 2))
        self.ids = np.concatenate([self.ids, self.next + np.arange(n_new)]); self.next += n_new
        self.X = np.concatenate([self.X, Xn]); self.age = np.concatenate([self.age, np.zeros(n_new, np.int64)])
        self.fyx = np.concatenate([self.fyx, yx_new]); self.fkf = np.concatenate([self.fkf, np.full(n_new, k, np.int32)])
        T = np.eye(4); T[0, 3] = -0.3 * k
        yx = self.project(self.X, k) + rng.normal(0, 0.3, (len(self.ids), 2))
        yx[self.age == 0] = yx_new
        f3 = self.age >= 2
        return T, yx, f3, np.where(f3[:, None], self.X, 0.0), self.ids.copy(), self.fyx.copy(), self.fkf.copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import slam_jl_amd as slam
    from slam_jl_amd import synthetic as syn
    S, R = args.streams, args.repeats
    ctx = slam.default_context(0)                                # no device: raises here, nothing is measured
    cam = syn.KITTI_CAM
    streams = [MonoStream(np.random.default_rng(100 + s), cam) for s in range(S)]
    ks_a, ks_b = slam.KeypointSet(S, CAP), slam.KeypointSet(S, CAP)
    km = slam.KeyframeMap(S, CAP, R=RING, mcap=MCAP)
    kf_cw = np.tile(np.eye(4), (S, NKF, 1, 1))
    m = {k: [] for k in ("set_wall", "map_wall", "poses", "temporal", "candidates", "triangulated", "set_removed")}
    ctx.prof_enable(True)
    for k in range(WARM + R):
        Tcw = np.tile(np.eye(4), (S, 1, 1))
        for s, st in enumerate(streams):
            Tcw[s], yx, f3, xyz, ids, fyx, fkf = st.keyframe(k)
            for ks in (ks_a, ks_b):
                ks.upload(s, yx, f3, xyz, ids)
            ks_a.upload_keyframe(s, fyx, np.ones(len(ids), dtype=bool))
            ks_a.upload_first(s, fyx, fkf, kf_count=k + 1)
            kf_cw[s, k % NKF] = Tcw[s]
        sp = slam.stream_params(S, Tcw=Tcw, cam=cam)
        ks_b.keyframe()
        km.add_keyframe(ks_b, sp)
        ctx.synchronize()
        Twc = np.stack([np.linalg.inv(T) for T in Tcw])
        before = int(ks_a.counts().sum())

        def set_route():
            t0 = time.perf_counter()
            ks_a.triangulate_temporal(slam.stream_params(S, cam=cam), kf_cw, Twc, np.full(S, k, np.int32), max_error=3.0)
            return (time.perf_counter() - t0) * 1e3

        def map_route():
            ctx.prof_reset()
            t0 = time.perf_counter()
            km.triangulate_temporal(cam, ks=ks_b, want_counts=False)
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3, ctx.prof_get("kfmap_tri_poses")[0], ctx.prof_get("kfmap_tri_temporal")[0]

        if k % 2:
            a = set_route(); b = map_route()
        else:
            b = map_route(); a = set_route()
        if k < WARM:
            continue
        pts = [km.download_points(s) for s in range(0, S, max(S // 4, 1))]       # (a sample of the streams: what the step left 3-D)
        m["set_wall"].append(a); m["map_wall"].append(b[0]); m["poses"].append(b[1]); m["temporal"].append(b[2])
        m["set_removed"].append(before - int(ks_a.counts().sum()))
        m["candidates"].append(float(np.mean([int(((st.age == 1)).sum()) for st in streams])))
        m["triangulated"].append(float(np.mean([int(p["is_3d"].sum()) for p in pts])))
    ctx.prof_enable(False)
    km.close(); ks_a.close(); ks_b.close()
    out = {"lib": os.path.basename(slam.LIB_PATH), "S": S, "cap": CAP, "keypoints_per_stream": NKP, "ring": RING, "table": MCAP, "host_pose_ring": NKF,
           "repeats": R, "warmup_keyframes": WARM, "candidates_per_stream": stat(m["candidates"]), "points_3d_in_map_per_sampled_stream": stat(m["triangulated"]),
           "set_route_removed_all_streams": stat(m["set_removed"]),
           "set_route_wall_ms": stat(m["set_wall"]), "map_route_wall_ms_with_synchronize": stat(m["map_wall"]),
           "k_kfm_tri_poses_ms": stat(m["poses"]), "k_kfm_tri_temporal_ms": stat(m["temporal"]),
           "note": "wall ms per key-frame step of all S streams; the set route includes its host table formation and its wait, the map route one synchronize"}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f_:
            f_.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
