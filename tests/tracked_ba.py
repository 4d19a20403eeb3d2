"""Local-BA windows gathered from tracked key-frames (test helper; never imported by the product).

A host-side map record of one stream is filled from the device keypoint lists after every key-frame step of
`benchlib.lockstep.run_lockstep_kpset(..., pose=True)` (its `diag` callback: `ks.download(s)` and `pst["Tcw"]`), and
`gather` / `update` restate the reference's local BA around it:

  gather  local_bundle_adjustment! + _get_ba_parameters (src/estimator.jl:317-335, :143-266)
  update  _update_ba_parameters! (src/estimator.jl:268-306)

so that the solver sees windows with the structure real key-frames give them -- points with one observer (triangulated at the
current key-frame), constant poses chosen by the covisibility rules, observers outside the window, tracking and triangulation
error -- instead of the synthetic generators' geometry.

The record is a model of the map manager, not the front end's own state: the BA results are written into the record only.  The
device lists are NOT written back (slam_kpset_upload resets the key-frame bookkeeping of a list; feeding BA results into the live
front end is the live-entry work).  What the reference would have done to the current frame -- an outlier observation of the
current key-frame removed from it, a map point removed -- is kept as the set `gone`: those ids are ignored in later lists.

`Record.mismatch` > 0 records a fixed share of each key-frame's observations a few pixels off (the rigid synthetic scene gives the
tracker nothing to mis-associate), so that the windows carry outliers the solver has to flag.

Orders that the reference takes from Julia dictionaries and sets (a key-frame's 3-D keypoint ids, a point's observers) are
ascending here; the order rules themselves (newest-first walk of the covisibility map, dense 1-based ids in first-encounter order)
are the reference's."""
from collections import OrderedDict

import numpy as np

MIN_COV_SCORE = 25                      # Params.min_cov_score (src/params.jl)
N_COVISIBLE = 5                         # local_bundle_adjustment!: up to 5 latest key-frames
# (min_cov_score, mismatch) of the records of streams 0..3 in the tracked tests.  Streams 0 and 1 keep the reference's threshold; in
# the synthetic runs every key-frame of a window shares hundreds of points with the newest, so no pose is ever constant by its score at
# 25 -- streams 2 and 3 raise the threshold (a sparser map's proportions) so that the oldest key-frames of a window are, and points seen
# by constant poses only appear.  The rigid scene has no tracking outliers: 1 % of the recorded observations are moved instead.
STREAM_CFG = [(25, 0.01), (25, 0.0), (400, 0.01), (700, 0.01)]


class MapPoint:
    __slots__ = ("xyz", "obs", "observed", "is_3d", "ba")

    def __init__(self, xyz, obs, observed, is_3d):
        self.xyz = np.asarray(xyz, dtype=np.float64).copy()
        self.obs = set(obs)             # observer key-frame ids
        self.observed = bool(observed)  # seen by the current frame
        self.is_3d = bool(is_3d)
        self.ba = False                 # position set by a BA (the device list's xyz no longer replaces it)


class KeyFrame:
    __slots__ = ("theta", "px")

    def __init__(self, theta, px):
        self.theta = np.asarray(theta, dtype=np.float64).copy()    # (RotZYX angles of Rcw, tcw)
        self.px = dict(px)                                          # keypoint id -> undistorted (y, x)


class Record:
    """The map of one stream: key-frames, map points, the current key-frame id and the ids the current frame has lost."""

    def __init__(self, cam, dist=None, min_cov_score=MIN_COV_SCORE, mismatch=0.0):
        self.cam = tuple(float(v) for v in cam)
        self.dist = None if dist is None or not np.any(dist) else tuple(float(v) for v in dist)
        self.min_cov_score = min_cov_score
        self.mismatch = mismatch        # share of a key-frame's observations recorded 7-9 px off (see add_keyframe)
        self.kfs = {}
        self.mps = {}
        self.cur = -1
        self.gone = set()

    def nb_3d(self, kfid):
        return sum(1 for k in self.kfs[kfid].px if k in self.mps and self.mps[k].is_3d)

    def ids_3d(self, kfid):
        """get_3d_keypoints_ids (frame.jl:198-208), ascending"""
        return sorted(k for k in self.kfs[kfid].px if k in self.mps and self.mps[k].is_3d)


def theta_of(Tcw):
    from oracle import oracle as orc
    T = np.asarray(Tcw, dtype=np.float64)
    return np.concatenate([orc.rotzyx_angles(T[:3, :3]), T[:3, 3]])


def add_keyframe(rec, kfid, Tcw, lst):
    """Record key-frame `kfid` at pose `Tcw` from a downloaded keypoint list (dict yx, ids, is_3d, xyz of KeypointSet.download)."""
    from oracle import oracle as orc
    assert kfid > rec.cur and kfid not in rec.kfs
    ids = np.asarray(lst["ids"], dtype=np.int64)
    keep = np.array([int(i) not in rec.gone for i in ids], dtype=bool)
    ids, yx, f3, xyz = ids[keep], np.asarray(lst["yx"])[keep], np.asarray(lst["is_3d"])[keep], np.asarray(lst["xyz"])[keep]
    if rec.dist is not None:
        yx = np.array([orc.undistort_point(rec.cam, rec.dist, p) for p in yx]).reshape(-1, 2)
    if rec.mismatch > 0:
        # the synthetic scene is rigid and the tracker never mis-associates a keypoint in it: a fixed share of the key-frame's observations
        # (chosen by a hash of kpid and kfid, so that every record of the same run picks the same ones) is recorded 7-9 px off instead
        h = (ids * 2654435761 + kfid * 40503) % 100003
        bad = h < rec.mismatch * 100003
        yx = yx.copy()
        yx[bad] += np.stack([7.0 + (h[bad] % 3), -8.0 + (h[bad] % 2)], axis=1)
    rec.kfs[kfid] = KeyFrame(theta_of(Tcw), {int(i): (float(p[0]), float(p[1])) for i, p in zip(ids, yx)})
    rec.cur = kfid
    seen = set(int(i) for i in ids)
    for mp in rec.mps.values():
        mp.observed = False
    for i, t3, x in zip(ids, f3, xyz):
        i = int(i)
        mp = rec.mps.get(i)
        if mp is None:
            rec.mps[i] = MapPoint(x, (kfid,), True, t3)
            continue
        mp.obs.add(kfid); mp.observed = True
        if t3 and not mp.ba:
            mp.xyz = np.asarray(x, dtype=np.float64).copy()
        mp.is_3d = mp.is_3d or bool(t3)
    assert all(rec.mps[i].observed for i in seen)


def is_bad(mp):
    """is_bad! (map_point.jl:155-161): a 3-D point with < 2 observers that the current frame does not see is demoted"""
    if len(mp.obs) < 2 and not mp.observed and mp.is_3d:
        mp.is_3d = False
        return True
    if not mp.obs and not mp.observed:
        mp.is_3d = False
        return True
    return False


def covisibility(rec, kfid):
    """update_frame_covisibility! counts (map_manager.jl:302-340): for every keypoint of the key-frame that is a map point, +1 per other observer"""
    cov = {}
    for k in rec.kfs[kfid].px:
        mp = rec.mps.get(k)
        if mp is None:
            continue
        for o in mp.obs:
            if o != kfid:
                cov[o] = cov.get(o, 0) + 1
    return cov


def remove_obs(rec, kpid, kfid):
    """remove_mappoint_obs! (map_manager.jl:224-): the key-frame loses the keypoint, the point the observer"""
    kf = rec.kfs.get(kfid)
    if kf is not None:
        kf.px.pop(kpid, None)
    mp = rec.mps.get(kpid)
    if mp is not None:
        mp.obs.discard(kfid)


def remove_mappoint(rec, kpid):
    """remove_mappoint! (map_manager.jl:139-168)"""
    mp = rec.mps.pop(kpid, None)
    if mp is None:
        return
    for o in mp.obs:
        if o in rec.kfs:
            rec.kfs[o].px.pop(kpid, None)
    if mp.observed:
        rec.gone.add(kpid)


def gather(rec, kfid=None):
    """The window of key-frame `kfid` (default: the current one) -> dict, or None when the key-frame has fewer than min_cov_score
    3-D keypoints.  Arrays as LocalBACache takes them (theta = [6P ; 3M], theta_const, pixels (O, 2) (y, x), 1-based ids) plus the
    bookkeeping update() needs: per observation its key-frame, map point and in_covmap; poses_remap, points_remap, bad."""
    kfid = rec.cur if kfid is None else kfid
    nb3 = rec.nb_3d(kfid)
    if nb3 < rec.min_cov_score:
        return None
    cov = covisibility(rec, kfid)
    cov[kfid] = nb3
    co = sorted(cov, reverse=True)[:N_COVISIBLE]
    covmap = OrderedDict((k, cov[k]) for k in co)
    minc = rec.min_cov_score
    poses = {}                           # kfid -> (order id, theta)
    constant = set()
    points = {}                          # kpid -> (order id, xyz)
    processed, bad = set(), set()
    obs = []                             # (pixel, pose order, point order, constant, in_covmap, kfid, kpid)
    poses_remap, points_remap = [], []
    for co_kfid, score in covmap.items():
        if co_kfid not in rec.kfs:
            continue
        if co_kfid > kfid or rec.nb_3d(co_kfid) == 0 or score == 0:
            continue
        if co_kfid not in poses and co_kfid not in constant:
            if score < minc or co_kfid == 0:
                constant.add(co_kfid)
                continue
        for kpid in rec.ids_3d(co_kfid):
            if kpid in processed:
                continue
            processed.add(kpid)
            mp = rec.mps.get(kpid)
            if mp is None:
                continue
            if is_bad(mp):
                bad.add(kpid)
                continue
            points[kpid] = (len(points) + 1, mp.xyz.copy())
            points_remap.append(kpid)
            for ob in sorted(mp.obs):
                if ob > kfid:
                    continue
                if ob not in rec.kfs or kpid not in rec.kfs[ob].px:
                    remove_obs(rec, kpid, ob)
                    continue
                in_covmap = ob in covmap
                is_const = ob == 0 or ob in constant or not in_covmap
                if not is_const and in_covmap:
                    is_const = covmap[ob] < minc
                if ob not in poses:
                    poses[ob] = (len(poses) + 1, rec.kfs[ob].theta.copy())
                    poses_remap.append(ob)
                    if is_const:
                        constant.add(ob)
                obs.append((rec.kfs[ob].px[kpid], poses[ob][0], points[kpid][0], is_const, in_covmap, ob, kpid))
    P, M, O = len(poses), len(points), len(obs)
    theta = np.empty(6 * P + 3 * M)
    tconst = np.zeros(P, dtype=np.uint8)
    done_p = np.zeros(P, dtype=bool)
    for kf_, (o, th) in poses.items():
        theta[6 * (o - 1):6 * o] = th
    for kp_, (o, x) in points.items():
        theta[6 * P + 3 * (o - 1):6 * P + 3 * o] = x
    for px, po, lo, c, _, _, _ in obs:
        if not done_p[po - 1]:
            done_p[po - 1] = True
            tconst[po - 1] = c
    return dict(kfid=kfid, covmap=covmap, theta=theta, theta_const=tconst,
                pixels=np.array([o[0] for o in obs], dtype=np.float64).reshape(O, 2),
                poses_ids=np.array([o[1] for o in obs], dtype=np.int64), points_ids=np.array([o[2] for o in obs], dtype=np.int64),
                obs_kf=np.array([o[5] for o in obs], dtype=np.int64), obs_kp=np.array([o[6] for o in obs], dtype=np.int64),
                obs_in_covmap=np.array([o[4] for o in obs], dtype=bool),
                poses_remap=np.array(poses_remap, dtype=np.int64), points_remap=np.array(points_remap, dtype=np.int64), bad=set(bad))


def update(rec, win, theta, outliers):
    """_update_ba_parameters! (estimator.jl:268-306): the solved theta and outlier flags of window `win` (from gather) into the record"""
    P = len(win["poses_remap"])
    bad = set(win["bad"])
    for i, k in enumerate(win["poses_remap"]):
        rec.kfs[int(k)].theta = np.array(theta[6 * i:6 * i + 6], dtype=np.float64)
    for i in np.flatnonzero(np.asarray(outliers, dtype=bool)):
        kf, kp = int(win["obs_kf"][i]), int(win["obs_kp"][i])
        if win["obs_in_covmap"][i]:
            remove_obs(rec, kp, kf)
        if kf == win["kfid"]:            # remove_obs_from_current_frame!
            mp = rec.mps.get(kp)
            if mp is not None:
                mp.observed = False
            rec.gone.add(kp)
        bad.add(kp)
    for i, kp in enumerate(win["points_remap"]):
        kp = int(kp)
        mp = rec.mps[kp]
        if is_bad(mp):
            remove_mappoint(rec, kp)
            bad.discard(kp)
        else:
            mp.xyz = np.array(theta[6 * P + 3 * i:6 * P + 3 * i + 3], dtype=np.float64)
            mp.ba = True
    for kp in bad:
        mp = rec.mps.get(kp)
        if mp is not None and is_bad(mp):
            remove_mappoint(rec, kp)


def structure(win):
    """What a window exercises: (P, free P, M, O, single-observation points of a free pose, points seen by constant poses only,
    constant poses other than key-frame 0)"""
    P = len(win["theta_const"])
    M = (len(win["theta"]) - 6 * P) // 3
    pi, li, c = win["poses_ids"] - 1, win["points_ids"] - 1, win["theta_const"].astype(bool)
    nobs = np.bincount(li, minlength=M)
    nfree = np.bincount(li, weights=(~c[pi]).astype(float), minlength=M)
    single_free = int(((nobs == 1) & (nfree == 1)).sum())
    const_only = int(((nobs > 0) & (nfree == 0)).sum())
    const_not0 = int(sum(1 for k, cc in zip(win["poses_remap"], c) if cc and k != 0))
    return dict(P=P, free=int((~c).sum()), M=M, O=len(pi), single_free=single_free, const_only=const_only, const_not0=const_not0)


def snapshot(rec):
    """Comparable state of a record: {kfid: theta}, {kpid: xyz}, {kpid: sorted observers}, sorted gone ids"""
    return ({k: f.theta.copy() for k, f in rec.kfs.items()}, {k: m.xyz.copy() for k, m in rec.mps.items()},
            {k: tuple(sorted(m.obs)) for k, m in rec.mps.items()}, tuple(sorted(rec.gone)))


def run_tracked(slam, syn, name, S, periods, on_keyframe, seed=0):
    """Run workload `name` (benchlib.lockstep.WORKLOADS) with S streams and the pose loop for 2 + `periods` key-frame periods; after every
    key-frame step call on_keyframe(kfid, Tcw (S, 4, 4), [list of stream s for s < S], camt)."""
    import torch
    from benchlib.lockstep import make_workload, run_lockstep_kpset
    wl = make_workload(slam, syn, name, seed=seed, streams=S)

    def diag(i, kf, pst, ks, ctx, off_now):
        if not kf:
            return
        lists = [ks.download(s, ctx=ctx) for s in range(S)]
        on_keyframe(pst["n_kf"] - 1, pst["Tcw"].copy(), lists, wl["camt"])

    return run_lockstep_kpset(slam, torch, 0, wl, periods, 2, 1, None, torch.device("cuda", 0), "host_u8", pose=True, diag=diag)
