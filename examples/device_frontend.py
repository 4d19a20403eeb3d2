#!/usr/bin/env python3
"""The reference's per-frame front-end (front_end.jl:60-113 + the mapper's stereo path, mapper.jl:51-66, 142-183) for S
lock-stepped stereo streams with every keypoint list resident in HBM -- the calls a host issues per frame:

    left frames  -> PyramidBatch.update_                                   (preprocess!)
    KeypointSet.flow_match      prior = projection of the map points under the predicted pose   (klt_tracking!)
    KeypointSet.compute_pose_5pt   epipolar outlier filter against the previous key-frame       (compute_pose_5pt!)
    KeypointSet.compute_pose       P3P RANSAC + PnP refinement -> the frame's pose              (compute_pose!)
    key-frames: detect -> keyframe -> right frames -> stereo_match -> triangulate -> triangulate_temporal   (create_keyframe!, mapper)
    --adaptive-keyframes: KeypointSet.frame_stats + keyframe_required after the pose                 (check_new_kf_required)
    --local-ba: after every key-frame step KeyframeMap.add_keyframe -> gather -> bundle_adjustment_batch_ -> update(ks)   (local_bundle_adjustment!)
    --map-filtering: after update(ks) KeyframeMap.filter drops the redundant key-frames of the ring                          (map_filtering!)
    --local-map-match: key-frames detect WITH describe; after add_keyframe KeyframeMap.add_descriptors -> local_map_match     (update_frame_covisibility! + match_local_map!)
    --device-ba: with --local-ba the step is KeyframeMap.add_keyframe -> local_ba(ks): emit, solve and update on the windows where they lie in HBM
    --merge: after local_map_match KeyframeMap.merge(ks) applies the match's pairs to the map and the lists, before the gather  (merge_matches)
    --descriptor-rows D: KeyframeMap.enable_descriptor_rows(D); a point keeps one row per key-frame, the match takes the minimum over all pairs of rows  (keyframes_descriptors)
    --local-map-history: KeyframeMap.enable_local_map_history; the match keeps every key-frame's local map and takes in the oldest covisible one's  (frame.local_map_ids)
    --map-triangulation: with --local-ba KeyframeMap.add_keyframe moves up behind the stereo triangulate and KeyframeMap.triangulate_temporal(ks) replaces KeypointSet.triangulate_temporal  (triangulate_temporal! on the map)

No host keypoint arrays anywhere; per frame the host receives S poses, S status words and S list lengths.  It is an
array-level driver, not SLAM (no relocalisation; the local-map match of --local-map-match is followed by its merges only with --merge): what it shows is that the seams compose -- on a rigid synthetic
scene the poses it returns are the camera motion.

With --local-ba the estimator's step runs too, on a key-frame map that lives in HBM beside the lists (slam_kfmap): every key-frame is recorded
from the lists, the windows of the streams' newest key-frames are gathered in slam_local_ba_batch's layout, solved in one batch, and the
solution goes back into the map AND the live lists -- the front end tracks refined landmarks from the next frame on.  Under
--adaptive-keyframes / --per-stream-keyframes the map calls run under the same selection as the key-frame seams.

With --map-filtering (requires --local-ba) the other half of the estimator's loop runs as well: after the update, map_filtering!
(estimator.jl:358-406) removes from each stream's ring the covisible key-frames most of whose 3-D points more than four key-frames observe
(Params.filtering_ratio), from key-frame --filter-from on (the reference's literal is 20).  A removed key-frame no longer enters later windows.

With --local-map-match (requires --local-ba) the mapper's last step before the estimator runs on the map too: the key-frame's new keypoints are
described on the device (KeypointSet.detect_describe), their descriptors go into the map (add_descriptors), and the local map of every stream's newest
key-frame -- the 3-D points of its covisible key-frames that it does not observe itself -- is staged and matched in HBM (local_map_match).  The pairs
(keypoint id, local-map point id) are reported per stream.  With --merge (requires --local-map-match) the pairs are applied where they lie in HBM
(KeyframeMap.merge: merge_matches -> merge_mappoints -> update_keypoint!) before the windows are gathered, and the per-stream counts are printed; on
the rigid scene the match finds no pair, so the flag shows the wiring and that a call without pairs changes nothing.
With --local-map-history (requires --local-map-match, combines with --merge) the map keeps the local map of every key-frame of its ring
(KeyframeMap.enable_local_map_history) and the match follows map_manager.jl:350-354 and mapper.jl:274-286: a point can be offered after every key-frame
that observes it has stopped being covisible with the newest one.  The rigid scene still yields no pair, and while every key-frame of the ring stays
covisible with the newest one the chain adds no point either: the flag shows the wiring (the stored sets can be read back with local_map_ids).

Key-frames are taken every `kf_every`-th frame, or, with --adaptive-keyframes, where the reference's rule asks for one
(front_end.jl:361-393 on the statistics of the lists, one S x 8 read-back per frame).  The streams are lock-stepped -- every launch is
shared -- so --adaptive-keyframes alone takes a key-frame FOR ALL streams when ANY stream requires one.  --per-stream-keyframes lets every
stream follow its own rule: the key-frame seams run under KeypointSet.selected(required), which restricts them to the streams that asked
(slam_kpset_select), and the key-frame bookkeeping (last key-frame, its nb_3d_kpts, its pose, the observer ring, the key-frame id) is per stream.
The right frames of such a key-frame are uploaded, built and matched for the streams that asked only: a COMPACT build into the first members of the
right batch (PyramidBatch.update_selected_) and a compact stereo match (stereo_match(..., compact=True)); --right-members K sizes that batch.

With --map-triangulation (requires --local-ba) the temporal triangulation reads the map instead of a host table of poses: the key-frame is recorded
right after the stereo triangulation, and every 2-D point of it is triangulated against its first observer as the map knows it NOW -- the smallest
key-frame id among the point's observers after every removal -- with the pose the last bundle adjustment left in the map, not the pose the key-frame was
taken with.  The kf_cw ring of the host is then not read; a rejected observation leaves the map while the list keeps the keypoint.

    python examples/device_frontend.py --frames 12 --streams 4 [--adaptive-keyframes | --per-stream-keyframes [--right-members K]]
        [--local-ba [--map-triangulation] [--device-ba] [--map-filtering [--filter-from K]]
         [--local-map-match [--merge] [--local-map-history] [--descriptor-rows D]]]
"""
import argparse
import contextlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slam_jl_amd as slam  # noqa: E402
from slam_jl_amd import synthetic as syn  # noqa: E402


def run(lefts, rights, cam, baseline, kf_every=4, max_keypoints=300, seed=0, ctx=None, verbose=False, adaptive=False, probe=None, per_stream=False, local_ba=False,
        map_filtering=False, filter_from=20, map_probe=None, local_map_match=False, merge=False, local_map_history=False, descriptor_rows=0, device_ba=False,
        map_triangulation=False, right_members=None, whole_right_build=False):
    """lefts / rights: per stream a list of float images in [0, 1] (H, W).  Returns per frame a dict with the S poses
    (world -> camera, world = the first frame's camera), status words, list lengths and the wall time.
    adaptive: frame 0 is a key-frame; after the pose of every later frame the lists' statistics (KeypointSet.frame_stats, flags = 1) go
    through keyframe_required, and a key-frame is taken for all streams when any stream requires one (kf_every is not used).  Those rows
    also carry kf_stats (S, 8), kf_required, kf_rule, frames_delta and prev_kf_nb_3d (the key-frame's nb_3d_kpts, from the statistics
    taken when it was created).  probe(frame, keypoint set, R_compensation (S, 3, 3)) is called right after the statistics are taken.
    per_stream (implies adaptive): frame 0 is a key-frame for all streams; afterwards stream s takes a key-frame exactly where keyframe_required
    says so for s -- the key-frame seams run on the selected streams only -- and `keyframe` of a row is an (S,) bool array.  Only the selected
    streams' right frames are uploaded; they are built compact into the first members of the right batch and matched compact.
    right_members (per_stream only; default S): the number of members of the right batch, K x 7 planes instead of S x 7.  When more streams ask for
    a key-frame than it holds (frame 0 with K < S, for one), that frame falls back to an ordinary whole-batch right build and match, in a full S-member
    batch made at the first such frame.  whole_right_build (per_stream only): every key-frame takes that whole-batch path -- the behaviour before
    the compact builds existed, kept for comparison.  Rows carry `right_build`: "compact" / "whole" at a key-frame of a per_stream run.
    local_ba: a KeyframeMap follows the key-frames; after the key-frame seams (same selection) the key-frame is added, the windows are gathered,
    solved by bundle_adjustment_batch_ and written back into the map and the lists.  Rows of key-frame steps carry `ba`: per solved window
    (stream, P, M, O, outliers, ssr before, ssr after).
    map_filtering (needs local_ba): after the update KeyframeMap.filter(params.filtering_ratio, params.min_cov_score, first_kfid=filter_from) runs
    for the same streams; those rows carry `removed`: per stream the key-frame ids it dropped.  map_probe(frame, stage, ...) is called around the
    map calls of a key-frame step: ("lists", ks, kf_mask, Tcw) before add_keyframe, ("added", km) after it, ("solved", wins) after the solve and
    before the update, ("filtered", km, removed) after the filter.
    local_map_match (needs local_ba): key-frames detect with describe, the descriptors follow the key-frame into the map, and before the gather
    KeyframeMap.local_map_match runs for the same streams; those rows carry `lmm`: (status (S,), pairs per stream, distances per stream).  map_probe
    is also called with ("described", desc, info, dcap) -- the device tensors detect_describe filled -- and ("matched", km, status, pairs, dist).
    merge (needs local_map_match): behind the match KeyframeMap.merge(ks) applies its pairs, taken where the match left them on the device; those rows
    carry `merged`: the (S, 4) counts (pairs applied, pairs skipped, observations renamed, status); map_probe is called with ("merged", km, counts).
    descriptor_rows (needs local_map_match): D > 0: KeyframeMap.enable_descriptor_rows(D) -- a point keeps one descriptor row per key-frame (at most D).
    local_map_history (needs local_map_match): KeyframeMap.enable_local_map_history() -- the map keeps every key-frame's local map, the match applies the
    replace-or-union rule and takes in the oldest covisible key-frame's stored set (mapper.jl:274-286); max_local is then the table's size (sets grow along
    that chain; status 2 cannot occur).  KeyframeMap.local_map_ids(s, kfid) reads a stored set back.
    device_ba (needs local_ba): the estimator step is add_keyframe -> KeyframeMap.local_ba(ks): the windows are emitted, solved (slam_local_ba_batch_dev) and
    applied where they lie in HBM; `ba` is built from the call's stats and KeyframeMap.last_windows(); map_probe's "solved" stage is not called.
    map_triangulation (needs local_ba): KeyframeMap.add_keyframe runs right behind the stereo triangulate (map_probe's "lists" and "added" stages with it) and
    KeyframeMap.triangulate_temporal(cam, ks=ks) stands where KeypointSet.triangulate_temporal stood; those rows carry `tri`: the (S, 4) counts (candidates,
    triangulated, observations removed, skipped), and map_probe is called with ("triangulated", km, counts).  Every other call is where it was."""
    if map_triangulation and not local_ba:
        raise ValueError("map_triangulation needs local_ba: the triangulation reads the local BA's key-frame map")
    if device_ba and not local_ba:
        raise ValueError("device_ba needs local_ba: it is the local BA's estimator step with the windows kept in HBM")
    if map_filtering and not local_ba:
        raise ValueError("map_filtering needs local_ba: the filter works on the local BA's key-frame map")
    if local_map_match and not local_ba:
        raise ValueError("local_map_match needs local_ba: the match works on the local BA's key-frame map")
    if merge and not local_map_match:
        raise ValueError("merge needs local_map_match: it applies the match's pairs")
    if local_map_history and not local_map_match:
        raise ValueError("local_map_history needs local_map_match: it is the match that keeps and reads the stored local maps")
    if descriptor_rows and not local_map_match:
        raise ValueError("descriptor_rows needs local_map_match: the rows are what the match is decided on")
    if right_members is not None and not (per_stream and 1 <= right_members <= len(lefts)):
        raise ValueError("right_members sizes the compact right batch of per_stream: 1 .. S members")
    adaptive = adaptive or per_stream
    import torch
    ctx = ctx or slam.default_context(0)
    S = len(lefts); n_frames = len(lefts[0])
    H, W = lefts[0][0].shape
    fx, fy, cx, cy = cam
    params = slam.Params(stereo=True, max_nb_keypoints=max_keypoints, map_filtering=map_filtering)
    camera = slam.Camera(fx, fy, cx, cy, height=H, width=W)
    ex = slam.Extractor.from_params(params, camera)
    ncell = ex.grid_resolution[0] * ex.grid_resolution[1]
    ks = slam.KeypointSet(S, max_keypoints + ncell + 8, ctx=ctx)
    km = slam.KeyframeMap(S, ks.cap, R=16, mcap=8192, ctx=ctx) if local_ba else None
    if local_map_match:
        km.enable_descriptors(ctx=ctx)
        if descriptor_rows:
            km.enable_descriptor_rows(descriptor_rows, ctx=ctx)
        if local_map_history:
            km.enable_local_map_history(ctx=ctx)
        dcap = ncell * -(-ex.max_points // ncell)
        desc = torch.zeros((S, dcap, 4), dtype=torch.int64, device="cuda"); info = torch.zeros((S, 2), dtype=torch.int64, device="cuda")
        cam10 = (fx, fy, cx, cy, 0.0, 0.0, 0.0, 0.0, float(H), float(W))
        torch.cuda.synchronize()
    prev = slam.PyramidBatch((H, W), levels=params.pyramid_levels, S=S, ctx=ctx)
    cur = slam.PyramidBatch((H, W), levels=params.pyramid_levels, S=S, ctx=ctx)
    rpyr = slam.PyramidBatch((H, W), levels=params.pyramid_levels, S=right_members if per_stream and right_members else S, ctx=ctx)
    rfull = rpyr if rpyr.S == S else None                                           # the whole-batch fallback's batch: made when first needed
    dev = lambda im: torch.from_numpy(np.ascontiguousarray(im.T)).cuda()          # Julia layout: column-major H x W
    T21 = np.eye(4); T21[0, 3] = -baseline                                          # left camera -> right camera
    Tcw = np.tile(np.eye(4), (S, 1, 1)); Tkf = Tcw.copy()
    NKF = 8; kf_cw = np.tile(np.eye(4), (S, NKF, 1, 1)); n_kf = np.zeros(S, np.int32)     # poses of the last key-frames (triangulate_temporal!'s observers), per stream
    sp_right = slam.stream_params(S, cam=cam, shift_yx=np.zeros((S, 2)))
    last_kf, prev_kf_nb_3d = np.zeros(S, np.int32), np.zeros(S, np.int32)      # adaptive: frame id and nb_3d_kpts of each stream's previous key-frame
    out = []
    for i in range(n_frames):
        t0 = time.perf_counter()
        prev, cur = cur, prev
        frames = [dev(lefts[s][i]) for s in range(S)]
        torch.cuda.synchronize()
        cur.update_([f.data_ptr() for f in frames], sigma=params.pyramid_sigma, ctx=ctx)
        status = np.zeros(S, np.int32); st5 = np.zeros(S, np.int32)
        if i > 0:
            # motion model: the last pose (constant-position prediction is enough for the prior of a 3-D keypoint)
            ks.flow_match(prev, cur, params, slam.stream_params(S, Tcw=Tcw, cam=cam), prior=1, ctx=ctx)
            # R_compensation = Rcw(key-frame) * Rwc(frame), front_end.jl:251
            Rc = np.tile(np.eye(4), (S, 1, 1))
            for s in range(S):
                Rc[s, :3, :3] = Tkf[s, :3, :3] @ Tcw[s, :3, :3].T
            Rt5, st5, n5, par, _ = ks.compute_pose_5pt(slam.stream_params(S, Tcw=Rc, cam=cam), min_parallax=5.0,
                                                       max_repr_error=params.max_reprojection_error, iters=64, seed=seed + 2 * i, ctx=ctx)
            poses, status, ninl, _ = ks.compute_pose(slam.stream_params(S, cam=cam), threshold=params.max_reprojection_error,
                                                     iters=128, seed=seed + 2 * i + 1, ctx=ctx)
            for s in range(S):
                if status[s]:
                    Tcw[s] = poses[s]
        kf_mask, decision = np.full(S, i % kf_every == 0), {}         # the streams that take a key-frame at this frame
        if adaptive:
            kf_mask = np.full(S, i == 0)
            if i > 0:                                                       # check_new_kf_required, front_end.jl:117
                Rc = np.tile(np.eye(4), (S, 1, 1))
                for s in range(S):
                    Rc[s, :3, :3] = Tkf[s, :3, :3] @ Tcw[s, :3, :3].T      # against the pose just computed
                stats = ks.frame_stats(slam.stream_params(S, Tcw=Rc, cam=cam), 1, ex.cell_size, (H, W), ctx=ctx)
                if probe is not None:
                    probe(i, ks, Rc[:, :3, :3].copy())
                fd = (i - last_kf).astype(np.int32)
                req, rule = slam.keyframe_required(stats, fd, prev_kf_nb_3d, np.ones(S, np.uint8), params, local_ba_on=False)
                kf_mask = req.copy() if per_stream else np.full(S, bool(req.any()))    # lock-step without per_stream: one stream's need is every stream's key-frame
                decision = dict(kf_stats=stats, kf_required=req, kf_rule=rule, frames_delta=fd, prev_kf_nb_3d=prev_kf_nb_3d.copy())
        if kf_mask.any():
            # the six key-frame seams act on the streams of kf_mask (all of them without per_stream: no selection is ever set then)
            with (ks.selected(kf_mask, ctx=ctx) if per_stream else contextlib.nullcontext()):
                if local_map_match:                                         # extract_keypoints! with describe (map_manager.jl:98-113)
                    ks.detect_describe(ex, cur, desc.data_ptr(), info.data_ptr(), dcap, ctx=ctx)
                else:
                    ks.detect(ex, cur, ctx=ctx)
                ks.keyframe(ctx=ctx)
                Tkf[kf_mask] = Tcw[kf_mask]
                kfid = n_kf.copy()                                          # per stream: the id of the key-frame being created
                for s in np.flatnonzero(kf_mask):
                    kf_cw[s, kfid[s] % NKF] = Tcw[s]
                n_kf[kf_mask] += 1
                if per_stream and not whole_right_build and int(kf_mask.sum()) <= rpyr.S:
                    # the right frames of the streams that asked, built into members 0 .. n_sel-1, matched through each stream's rank
                    rframes = {s: dev(rights[s][i]) for s in np.flatnonzero(kf_mask)}
                    torch.cuda.synchronize()
                    rptrs = [rframes[s].data_ptr() if s in rframes else 0 for s in range(S)]
                    rpyr.update_selected_(rptrs, kf_mask, sigma=params.pyramid_sigma, ctx=ctx, target_only=True)
                    ks.stereo_match(cur, rpyr, params, sp_right, prior=2, ctx=ctx, compact=True)
                    decision["right_build"] = "compact"
                else:
                    if rfull is None:                                       # more streams asked than the compact batch holds
                        rfull = slam.PyramidBatch((H, W), levels=params.pyramid_levels, S=S, ctx=ctx)
                    rframes = [dev(rights[s][i]) for s in range(S)]
                    torch.cuda.synchronize()
                    rfull.update_([f.data_ptr() for f in rframes], sigma=params.pyramid_sigma, ctx=ctx, target_only=True)   # only matched INTO
                    ks.stereo_match(cur, rfull, params, sp_right, prior=2, ctx=ctx)
                    if per_stream:
                        decision["right_build"] = "whole"
                Twc = np.stack([np.linalg.inv(Tcw[s]) for s in range(S)])
                ks.triangulate(cam, cam, T21, Twc, max_error=params.max_reprojection_error, ctx=ctx)
                notify = map_probe or (lambda *a: None)
                if map_triangulation:                                       # the map's copy of the key-frame first, as the reference's mapper has it
                    notify(i, "lists", ks, kf_mask.copy(), Tcw.copy())
                    km.add_keyframe(ks, slam.stream_params(S, Tcw=Tcw, cam=cam), ctx=ctx)
                    notify(i, "added", km)
                if (kfid[kf_mask] > 0).any():                               # mapper.jl:86: 2-D keypoints left over, against their first observers
                    if map_triangulation:                                   # the observers, their pixels and their refined poses are the map's
                        decision["tri"] = km.triangulate_temporal(cam, ks=ks, max_error=params.max_reprojection_error, ctx=ctx)
                        notify(i, "triangulated", km, decision["tri"])
                    else:
                        ks.triangulate_temporal(slam.stream_params(S, cam=cam), kf_cw, Twc, kfid, max_error=params.max_reprojection_error, ctx=ctx)
                if km is not None:                                          # local_bundle_adjustment! (estimator.jl:317-347) of the streams that took the key-frame
                    if not map_triangulation:
                        notify(i, "lists", ks, kf_mask.copy(), Tcw.copy())
                        km.add_keyframe(ks, slam.stream_params(S, Tcw=Tcw, cam=cam), ctx=ctx)
                        notify(i, "added", km)
                    if local_map_match:                                     # update_frame_covisibility! + match_local_map! (mapper.jl:118-133), before add_new_kf!
                        km.add_descriptors(desc.data_ptr(), info.data_ptr(), dcap, ctx=ctx)
                        notify(i, "described", desc, info, dcap)
                        decision["lmm"] = km.local_map_match(cam10, ex.cell_size, params.max_projection_distance, params.max_descriptor_distance,
                                                             max_local=km.mcap if local_map_history else 10 * max_keypoints, ctx=ctx)
                        notify(i, "matched", km, *decision["lmm"])
                        if merge:                                           # merge_matches (mapper.jl:296-310): before the estimator reads the map
                            decision["merged"] = km.merge(ks, ctx=ctx)
                            notify(i, "merged", km, decision["merged"])
                    if device_ba:                                           # the same step without the windows' trip through the host
                        ba_status, ba_stats = km.local_ba(params.min_cov_score, cam, ks=ks, ctx=ctx)
                        pmo = km.last_windows()
                        wins = []
                        decision["ba"] = [(s_, int(pmo[s_, 0]), int(pmo[s_, 1]), int(pmo[s_, 2]), int(ba_stats[s_, 5]), float(ba_stats[s_, 0]), float(ba_stats[s_, 2]))
                                          for s_ in range(S) if ba_status[s_] == 0]
                    else:
                        wins, _ = km.gather(params.min_cov_score, ctx=ctx)
                        if wins:
                            slam.bundle_adjustment_batch_([w.cache for w in wins], cam, ctx=ctx)
                            notify(i, "solved", wins)
                            km.update(wins, ks=ks, ctx=ctx)
                    if params.map_filtering:                                # map_filtering! (estimator.jl:358-406), the estimator's next step
                        decision["removed"] = km.filter(params.filtering_ratio, params.min_cov_score, first_kfid=filter_from, ctx=ctx)
                        notify(i, "filtered", km, decision["removed"])
                    if not device_ba:
                        decision["ba"] = [(w.stream, w.cache.n_poses, w.cache.n_points, len(w.cache.poses_ids), int(w.cache.outliers.sum()),
                                           w.cache.stats["ssr_init"], w.cache.stats["ssr_final"]) for w in wins]
            if adaptive:                                                    # the key-frame's own nb_3d_kpts, after the mapper's triangulations
                last_kf[kf_mask] = i
                nb_3d = ks.frame_stats(slam.stream_params(S, cam=cam), 0, ex.cell_size, (H, W), ctx=ctx)[:, 1].astype(np.int32)
                prev_kf_nb_3d[kf_mask] = nb_3d[kf_mask]                     # refreshed only for the streams that took the key-frame
        cnt = ks.counts(ctx=ctx)
        row = dict(frame=i, keyframe=kf_mask.copy() if per_stream else bool(kf_mask.any()), poses=Tcw.copy(), status=status.copy(), status_5pt=np.asarray(st5).copy(),
                   counts=cnt.copy(), ms=(time.perf_counter() - t0) * 1e3)
        row.update(decision)
        out.append(row)
        if verbose:
            print(f"frame {i:3d} kf={row['keyframe']!s:5} keypoints {cnt.tolist()} pose ok {status.tolist()} 5pt ok {np.asarray(st5).tolist()} "
                  f"t = {np.round(Tcw[0][:3, 3], 3).tolist()} {row['ms']:.2f} ms")
            for s_, P_, M_, O_, no_, e0_, e1_ in row.get("ba", []):
                print(f"          local BA stream {s_}: window of {P_} poses, {M_} points, {O_} observations; {no_} outliers, ssr {e0_:.3f} -> {e1_:.3f}")
            if "tri" in row:
                print(f"          temporal triangulation on the map: candidates {row['tri'][:, 0].tolist()}, triangulated {row['tri'][:, 1].tolist()}, "
                      f"observations removed {row['tri'][:, 2].tolist()}, skipped {row['tri'][:, 3].tolist()}")
            if "lmm" in row:
                print(f"          local-map match: status {row['lmm'][0].tolist()}, pairs per stream {[len(p) for p in row['lmm'][1]]}")
            if "merged" in row:
                print(f"          merge: pairs applied {row['merged'][:, 0].tolist()}, skipped {row['merged'][:, 1].tolist()}, observations renamed {row['merged'][:, 2].tolist()}")
            if "removed" in row:
                print(f"          map filtering: removed key-frames {row['removed']}")
    n3 = [int(ks.download(s)["is_3d"].sum()) for s in range(S)]
    if km is not None:
        km.close()
    ks.close()
    return out, n3


def synthetic_scene(S, n_frames, shape=(200, 320), disparity=8.0, seed=0):
    """A fronto-parallel textured plane seen by cameras translating parallel to it: per stream left / right frames, the
    per-frame image offsets (y, x) in pixels, and the plane's depth Z = fx b / d (the image shift of o pixels is the camera
    translation -o Z / f)."""
    lefts, rights, offs = [], [], []
    for s in range(S):
        L, R, flows = syn.stereo_stream(shape, n_frames, seed=seed + s, step=(1.1 + 0.3 * s, -1.6 + 0.2 * s), disparity=disparity)
        lefts.append(L); rights.append(R); offs.append(np.asarray(flows, dtype=np.float64))
    return lefts, rights, offs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--adaptive-keyframes", action="store_true", help="take key-frames where check_new_kf_required asks for one (any stream), not every 4th frame")
    ap.add_argument("--per-stream-keyframes", action="store_true", help="every stream takes its key-frames where check_new_kf_required asks for one for THAT stream (implies --adaptive-keyframes)")
    ap.add_argument("--right-members", type=int, default=None, metavar="K",
                    help="with --per-stream-keyframes: members of the right pyramid batch (default: one per stream); a frame at which more streams take "
                         "a key-frame falls back to a whole-batch right build")
    ap.add_argument("--local-ba", action="store_true", help="run the estimator's local BA after every key-frame step, on a key-frame map in HBM; the lists take the refined landmarks")
    ap.add_argument("--device-ba", action="store_true", help="with --local-ba: the estimator step in one call with the windows kept in HBM (KeyframeMap.local_ba), not gather -> solve -> update through the host")
    ap.add_argument("--map-filtering", action="store_true", help="after every local BA drop the redundant key-frames of the map (map_filtering!); requires --local-ba")
    ap.add_argument("--local-map-match", action="store_true", help="describe the key-frames' new keypoints and match each stream's local map against them on the key-frame map (match_local_map!); requires --local-ba")
    ap.add_argument("--merge", action="store_true", help="apply the local-map match's pairs to the map and the lists (merge_matches); requires --local-map-match")
    ap.add_argument("--descriptor-rows", type=int, default=0, metavar="D", help="keep one descriptor row per key-frame and point, at most D = 2 .. 8 (keyframes_descriptors): merges hand rows over, removed observations drop theirs, the match reads all of them; requires --local-map-match")
    ap.add_argument("--local-map-history", action="store_true", help="keep every key-frame's local map on the device and let the match take in the oldest covisible key-frame's (frame.local_map_ids, match_local_map!); requires --local-map-match")
    ap.add_argument("--map-triangulation", action="store_true", help="triangulate the key-frame's 2-D points from the key-frame map (its first observers as they are now, its refined poses) instead of the host's pose table; requires --local-ba")
    ap.add_argument("--filter-from", type=int, default=20, help="first key-frame id at which the filter acts (the reference's literal 20)")
    ap.add_argument("--replay-dir", default=None, help="write stream s's camera positions to DIR/stream_s as a ReplaySaver dump (src/io/saver.jl)")
    args = ap.parse_args()
    if args.right_members is not None and not args.per_stream_keyframes:
        ap.error("--right-members requires --per-stream-keyframes")
    if args.device_ba and not args.local_ba:
        ap.error("--device-ba requires --local-ba")
    if args.map_filtering and not args.local_ba:
        ap.error("--map-filtering requires --local-ba")
    if args.map_triangulation and not args.local_ba:
        ap.error("--map-triangulation requires --local-ba")
    if args.local_map_match and not args.local_ba:
        ap.error("--local-map-match requires --local-ba")
    if args.merge and not args.local_map_match:
        ap.error("--merge requires --local-map-match")
    if args.local_map_history and not args.local_map_match:
        ap.error("--local-map-history requires --local-map-match")
    if args.descriptor_rows and not args.local_map_match:
        ap.error("--descriptor-rows requires --local-map-match")
    cam, baseline, disparity = syn.KITTI_CAM, 0.54, 8.0
    lefts, rights, offs = synthetic_scene(args.streams, args.frames, disparity=disparity)
    out, n3 = run(lefts, rights, cam, baseline, verbose=True, adaptive=args.adaptive_keyframes, per_stream=args.per_stream_keyframes, local_ba=args.local_ba,
                  map_filtering=args.map_filtering, filter_from=args.filter_from, local_map_match=args.local_map_match, merge=args.merge,
                  local_map_history=args.local_map_history, descriptor_rows=args.descriptor_rows, device_ba=args.device_ba,
                  map_triangulation=args.map_triangulation, right_members=args.right_members)
    Z = cam[0] * baseline / disparity
    for s in range(args.streams):
        o = offs[s][-1] - offs[s][0]
        want = np.array([o[1] * Z / cam[0], o[0] * Z / cam[1], 0.0])
        got = out[-1]["poses"][s][:3, 3]
        print(f"stream {s}: translation {np.round(got, 3).tolist()} m, expected {np.round(want, 3).tolist()} m (plane at {Z:.1f} m), {n3[s]} map points")
        if args.local_ba:
            n_win = sum(1 for r in out for w in r.get("ba", []) if w[0] == s)
            print(f"stream {s}: {n_win} local-BA windows solved, motion error {np.abs(got - want).max():.4f} m")
        if args.map_triangulation:
            print(f"stream {s}: the map triangulated {sum(int(r['tri'][s, 1]) for r in out if 'tri' in r)} points and removed {sum(int(r['tri'][s, 2]) for r in out if 'tri' in r)} observations")
        if args.local_map_match:
            print(f"stream {s}: local-map match found {sum(len(r['lmm'][1][s]) for r in out if 'lmm' in r)} pairs over {sum(1 for r in out if 'lmm' in r)} key-frames")
        if args.merge:
            print(f"stream {s}: merge applied {sum(int(r['merged'][s, 0]) for r in out if 'merged' in r)} pairs, renamed {sum(int(r['merged'][s, 2]) for r in out if 'merged' in r)} observations")
        if args.map_filtering:
            print(f"stream {s}: map filtering removed key-frames {sorted(k for r in out for k in r.get('removed', [[]] * args.streams)[s])}")
    if args.replay_dir:
        import os
        for s in range(args.streams):
            saver = slam.ReplaySaver()                      # set_frame_wc!(saver, frame id, wc) as SlamManager does after every frame
            for r in out:
                saver.set_frame_wc(r["frame"], np.linalg.inv(r["poses"][s]))
            saver.save(os.path.join(args.replay_dir, f"stream_{s}"))
        print(f"wrote positions.bson / ids.bson for {args.streams} streams under {args.replay_dir}")
    ms = np.array([r["ms"] for r in out[1:]])
    print(f"median {np.median(ms):.2f} ms per step of {args.streams} frames (wall, incl. the host -> device frame copies)")


if __name__ == "__main__":
    main()
