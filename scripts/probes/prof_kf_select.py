"""The key-frame sequence of a lock-stepped host -- detect -> keyframe -> stereo_match -> triangulate on the device-resident lists -- at the
throughput shape, without a selection and with 128, 64, 16, 1 and 0 streams selected (slam_kpset_select): what a key-frame costs when only
some streams need one.

Shape: S = 128 streams, 370 x 1226, max_nb_keypoints = 1000, cap 1400 (prof_frame_stats.py's set).  Every repeat starts from the same kind of
lists: a cull (slam_kpset_remove, 30 % of the selected streams' slots, outside the timed window) takes the lists back to about 700 keypoints, the
detection then refills them to about 1000.  Timed: a host clock from the first enqueue to the return of the context's synchronise behind the
last one (the seams only enqueue), after warm-up; median of `--repeats` with min-max.  The selected streams are spread evenly over 0 .. S-1.

--no-select runs the no-selection leg alone and never touches the selection calls: that leg uses only seams that existed before them, so the
same script times the parent commit (run it there, alternating with this tree, in one session on one machine).

--right-build times the other half of such a key-frame instead: the right-pyramid build (8-bit frames, target-only) + the stereo match, at 128, 64, 16
and 1 streams selected -- "whole": slam_pyr_update_batch_u8_dev of all S members + slam_kpset_stereo_match under the selection (what a per-stream
key-frame cost before the compact builds), "compact": slam_pyr_update_batch_sel_u8_dev of the selected streams + slam_kpset_stereo_match_compact.
Same clock (first enqueue to the return of the synchronise), same statistics; the lists are detected once and matched again every repeat.  Per count
the first compact build (its launch graph is made then) is timed on its own, beside the steady build.  --whole-only runs the whole-batch legs alone
and calls nothing newer than the selection: the same script times the parent commit.

    python scripts/probes/prof_kf_select.py [--streams 128] [--repeats 25] [--no-select] [--tag NAME] [--out profiles/kf_select_s128.json]
    python scripts/probes/prof_kf_select.py --right-build [--whole-only] [--tag NAME] [--out profiles/kf_select_right_s128.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
CAP, MAXKP, CULL = 1400, 1000, 0.3


def stat(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--no-select", action="store_true")
    ap.add_argument("--right-build", action="store_true")
    ap.add_argument("--whole-only", action="store_true")
    ap.add_argument("--tag", default="this tree")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import slam_jl_amd as slam
    from slam_jl_amd import synthetic as syn
    S, R = args.streams, args.repeats
    ctx = slam.default_context(0)                                # no device: raises here, nothing is measured
    H, W = syn.SHAPES["kitti05"]
    params = slam.Params(stereo=True, max_nb_keypoints=MAXKP)
    ex = slam.Extractor.from_params(params, slam.Camera(*syn.KITTI_CAM, height=H, width=W))
    left, right, _ = syn.stereo_stream("kitti05", 2, seed=0, disparity=12.4)
    ld = [torch.from_numpy(np.ascontiguousarray(im.T)).cuda() for im in left]
    rd = [torch.from_numpy(np.ascontiguousarray(im.T)).cuda() for im in right]
    torch.cuda.synchronize()
    lp = slam.PyramidBatch((H, W), levels=params.pyramid_levels, S=S)
    rp = slam.PyramidBatch((H, W), levels=params.pyramid_levels, S=S)
    lp.update_([ld[s % 2].data_ptr() for s in range(S)]); rp.update_([rd[s % 2].data_ptr() for s in range(S)])
    ctx.synchronize()
    sps = slam.stream_params(S, cam=syn.KITTI_CAM, shift_yx=np.tile([0.0, -12.4], (S, 1)))
    T21 = np.eye(4); T21[0, 3] = -0.54
    rng = np.random.default_rng(3)

    def sequence(ks):
        ks.detect(ex, lp)
        ks.keyframe()
        ks.stereo_match(lp, rp, params, sps, prior=2)
        ks.triangulate(syn.KITTI_CAM, syn.KITTI_CAM, T21, np.eye(4), max_error=3.0)

    def leg(name, mask):
        """mask None: no selection call at all"""
        ks = slam.KeypointSet(S, CAP)
        if mask is not None:
            ks.select(mask)
        on = np.ones(S, bool) if mask is None else np.asarray(mask, bool)
        flags = ((rng.random((S, CAP)) < CULL) & on[:, None]).astype(np.uint8)
        fdev = torch.from_numpy(flags).cuda(); torch.cuda.synchronize()
        times, before, after = [], None, None
        for it in range(5 + R):                                  # 5 warm-up rounds: code objects, scratch, the lists' steady state
            ks.remove(fdev.data_ptr())
            before = ks.counts()                                 # (synchronises)
            t0 = time.perf_counter()
            sequence(ks)
            ctx.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if it >= 5:
                times.append(dt)
            after = ks.counts()
        n_on = int(on.sum())
        rec = {"leg": name, "selected": None if mask is None else n_on, "wall_ms": stat(times),
               "keypoints_before_mean": float(before[on].mean()) if n_on else 0.0, "keypoints_after_mean": float(after[on].mean()) if n_on else 0.0}
        if mask is not None and n_on < S:
            assert (after[~on] == 0).all()                       # the unselected streams' lists stayed empty
        ks.close()
        return rec

    def right_legs():
        r8 = [torch.from_numpy(np.ascontiguousarray((np.clip(im, 0, 1) * 255).round().astype(np.uint8).T)).cuda() for im in right]
        torch.cuda.synchronize()
        ptrs = [r8[s % 2].data_ptr() for s in range(S)]
        legs = []
        for k in (S, S // 2, S // 8, 1):
            mask = np.zeros(S, np.uint8)
            mask[np.linspace(0, S - 1, k).round().astype(int)] = 1
            for compact in ([False] if args.whole_only else [False, True]):
                ks = slam.KeypointSet(S, CAP)
                ks.detect(ex, lp); ks.keyframe()                  # about 1000 2-D keypoints per stream; a stereo match leaves the lists as they are
                ks.select(mask)
                n_kp = float(ks.counts()[mask != 0].mean())

                def build():
                    if compact:
                        rp.update_selected_(ptrs, mask, u8=True, target_only=True, sync=False)
                    else:
                        rp.update_(ptrs, u8=True, target_only=True, sync=False)

                t0 = time.perf_counter(); build(); ctx.synchronize()
                first_ms = (time.perf_counter() - t0) * 1e3       # a member count not built before: the launch graph is made here
                both, alone = [], []
                for it in range(5 + R):
                    t0 = time.perf_counter()
                    build()
                    ks.stereo_match(lp, rp, params, sps, prior=2, **({"compact": True} if compact else {}))
                    ctx.synchronize()
                    t1 = time.perf_counter()
                    build(); ctx.synchronize()
                    t2 = time.perf_counter()
                    if it >= 5:
                        both.append((t1 - t0) * 1e3); alone.append((t2 - t1) * 1e3)
                matched = float(np.mean([ks.download(int(s))["has_stereo"].mean() for s in np.flatnonzero(mask)[:4]]))
                legs.append({"leg": f"{k} of {S} selected, {'compact' if compact else 'whole'} right build", "selected": k, "compact": compact,
                             "build_and_match_ms": stat(both), "build_alone_ms": stat(alone), "first_build_ms": round(first_ms, 4),
                             "keypoints_mean": n_kp, "stereo_matched_fraction": round(matched, 4)})
                ks.close()
        return legs

    if args.right_build:
        rec = {"lib": os.path.basename(slam.LIB_PATH), "tag": args.tag, "S": S, "cap": CAP, "max_nb_keypoints": MAXKP, "shape": [H, W], "repeats": R,
               "sequence": "right build (8-bit frames, target-only) -> stereo_match", "legs": right_legs()}
        print(json.dumps(rec))
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(rec, indent=1) + "\n")
        return
    rec = {"lib": os.path.basename(slam.LIB_PATH), "tag": args.tag, "S": S, "cap": CAP, "max_nb_keypoints": MAXKP, "shape": [H, W], "repeats": R,
           "sequence": "detect -> keyframe -> stereo_match -> triangulate", "legs": [leg("no selection", None)]}
    if not args.no_select:
        for k in (S, S // 2, S // 8, 1, 0):
            mask = np.zeros(S, np.uint8)
            if k:
                mask[np.linspace(0, S - 1, k).round().astype(int)] = 1
            assert int(mask.sum()) == k
            rec["legs"].append(leg(f"{k} of {S} selected", mask))
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
