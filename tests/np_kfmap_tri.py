"""Temporal triangulation on the bounded key-frame map (test helper; never imported by the product): the model of slam_kfmap_triangulate_temporal.

triangulate_temporal(m, cam, lst) restates triangulate_temporal! (src/mapper.jl:185-262) with update_mappoint! and remove_mappoint_obs!
(src/map_manager.jl:224-292) over an np_kfmap.Map; the arithmetic (pair) is numpy f64 written from those lines alone.  With k the newest key-frame
(slot r0), every live observation of its slab, in slab order:

  1  skipped, not a candidate: its point is missing (the entry carries another id), dead, or 3-D already (get_2d_keypoints, :208-211; no
     remove_mappoint_obs! clean-up for a missing point, as elsewhere in the map)
  2  FEW: fewer than two observers (:215); SELF: the first observer -- the smallest key-frame id among the mask's bits whose slot holds a key-frame --
     is k itself (:217)
  3  ABSENT: the first observer's slab does not hold the id alive (:234-235)
  4  rel_pose = observer.cw * frame.wc from the two thetas, rel_pose_inv by the closed-form rigid inverse, P2 = K rel_pose_inv, observer.wc
  5  parallax, DLT, the four gates; a failed gate counts only when the parallax exceeds min_parallax
  6  ACCEPTED: xyz = observer.wc X, F_3D set (not F_BA); with a list, the slot that carries the id takes xyz and is_3d
  7  REMOVED: the newest slab's observation becomes a tombstone, the point loses bit r0; THE LIST KEEPS THE KEYPOINT
  8  counts = (candidates after rule 1, accepted, removed, skipped by rules 2-3)

Per candidate the model returns the decision code, the observer's key-frame id and pixel, and `margin`: the smallest distance of any gate quantity to
its threshold (the two depths against min_depth, the two reprojection errors against max_error, the parallax against min_parallax), all five whatever
the gates' short cuts, plus `bz`, the z component of the rotated bearing the parallax divides by (the scripts keep it away from zero).

`mutant` breaks one rule, for the tests that show the scenes can tell: "largest" (the first observer is the largest id), "one" (one observer
suffices), "always" (a failed gate removes whatever the parallax), "newest_pose" (the world point goes through the newest key-frame's pose)."""
import math

import numpy as np

import np_kfmap as npk
import np_kfmap_local_map as nl

MUTANTS = ("largest", "one", "always", "newest_pose")
FEW, SELF, ABSENT, ACCEPTED, REMOVED = 1, 2, 3, 4, 5


def se3_inv(T):
    """inv(SE3, T) in closed form: [R' | -R' t]"""
    O = np.eye(4)
    O[:3, :3] = T[:3, :3].T
    O[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return O


def observer_mats(theta_ob, theta_fr):
    """mapper.jl:226-231 from the two key-frames' parameters -> (rel_pose, rel_pose_inv, observer.wc)"""
    Tob, Tfr = nl.tcw_of(theta_ob), nl.tcw_of(theta_fr)
    rel = Tob @ se3_inv(Tfr)
    return rel, se3_inv(rel), se3_inv(Tob)


def first_observer(observers, mutant=None):
    """observers: the key-frame ids that observe the point -> the first (None: the candidate is skipped as FEW)"""
    if len(observers) < (1 if mutant == "one" else 2):
        return None
    return max(observers) if mutant == "largest" else min(observers)


def pair(cam, rel, rel_inv, obup, kpup, max_error=3.0, min_depth=0.1, min_parallax=20.0, mutant=None):
    """mapper.jl:236-258 for one pair of undistorted pixels (y, x) -> dict(ok, left (4,), parallax, margin, bz)"""
    fx, fy, cx, cy = cam
    K = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    P1, P2 = K, K @ rel_inv
    project = lambda X: np.array([fy * X[1] / X[2] + cy, fx * X[0] / X[2] + cx])
    b = rel[:3, :3] @ np.array([(kpup[1] - cx) / fx, (kpup[0] - cy) / fy, 1.0])          # R(rel_pose) * kp.position
    with np.errstate(all="ignore"):
        parallax = float(np.linalg.norm(np.asarray(obup) - project(b)))
        x1, y1, x2, y2 = obup[1], obup[0], kpup[1], kpup[0]
        A = np.stack([x1 * P1[2] - P1[0], y1 * P1[2] - P1[1], x2 * P2[2] - P2[0], y2 * P2[2] - P2[1]])
        _, V = np.linalg.eigh(A.T @ A)                           # RecoverPose.triangulate: the eigenvector of the smallest eigenvalue
        left = V[:, 0] / V[3, 0]
        right = rel_inv @ left
        lrepr = float(np.linalg.norm(project(left[:3]) - np.asarray(obup)))
        rrepr = float(np.linalg.norm(project(right[:3]) - np.asarray(kpup)))
    gated = parallax > min_parallax or mutant == "always"
    fail = left[2] < min_depth or right[2] < min_depth or lrepr > max_error or rrepr > max_error
    dists = [abs(left[2] - min_depth), abs(right[2] - min_depth), abs(lrepr - max_error), abs(rrepr - max_error), abs(parallax - min_parallax)]
    margin = min(d for d in dists if not math.isnan(d)) if not all(math.isnan(d) for d in dists) else 0.0
    return dict(ok=not (fail and gated), fail=bool(fail), left=left, parallax=parallax, margin=float(margin), bz=float(b[2]))


def triangulate_temporal(m, cam, lst=None, max_error=3.0, min_depth=0.1, min_parallax=20.0, mutant=None):
    """-> dict(counts (4,), cand: one dict per candidate in slab order, list: the list as the device leaves it (None without one))"""
    out_list = None if lst is None else {k: np.asarray(v).copy() for k, v in lst.items()}
    counts, cand = np.zeros(4, dtype=np.int32), []
    k = m.cur
    if k < 0:
        return dict(counts=counts, cand=cand, list=out_list)
    r0 = k % m.R
    for i in range(int(m.n[r0])):
        if not m.live[r0, i]:
            continue
        kpid = int(m.ids[r0, i])
        e = m.entry(kpid)
        if e is None or m.flags[e] & npk.F_3D:                   # rule 1
            continue
        counts[0] += 1
        c = dict(id=kpid, code=0, observer=-1, obup=None, kpup=m.upx[r0, i].copy(), margin=math.inf, bz=1.0, xyz=None)
        cand.append(c)
        ob = first_observer(m.observers(e), mutant)              # rule 2
        if ob is None or ob == k:
            c["code"] = FEW if ob is None else SELF
            counts[3] += 1
            continue
        b = m.slot(ob)
        j = m.find_live(b, kpid)                                 # rule 3
        c["observer"] = ob
        if j is None:
            c["code"] = ABSENT
            counts[3] += 1
            continue
        rel, rel_inv, wob = observer_mats(m.theta[b], m.theta[r0])
        c["obup"] = m.upx[b, j].copy()
        r = pair(cam, rel, rel_inv, c["obup"], c["kpup"], max_error, min_depth, min_parallax, mutant)
        c.update(margin=r["margin"], bz=r["bz"], parallax=r["parallax"], fail=r["fail"], rel_inv=rel_inv, wob=wob)
        if r["ok"]:                                              # update_mappoint!
            world = ((se3_inv(nl.tcw_of(m.theta[r0])) if mutant == "newest_pose" else wob) @ r["left"])[:3]      # project_camera_to_world(observer_kf, .)
            m.xyz[e] = world; m.flags[e] |= npk.F_3D
            c["code"], c["xyz"] = ACCEPTED, world.copy()
            counts[1] += 1
            if out_list is not None:
                hit = np.flatnonzero(out_list["ids"] == kpid)
                if len(hit):
                    out_list["xyz"][hit[0]] = world; out_list["is_3d"][hit[0]] = True
        else:                                                    # remove_mappoint_obs!(map, id, k): the list keeps the keypoint
            m.live[r0, i] = False
            m.mask[e] &= ~(1 << r0)
            c["code"] = REMOVED
            counts[2] += 1
    return dict(counts=counts, cand=cand, list=out_list)


# ---- the literal restatement on tests/tracked_ba.py's unbounded Record: dicts and sets only ---------------------------------------------------------------
def restated(rec, cam, max_error=3.0, min_depth=0.1, min_parallax=20.0):
    """triangulate_temporal! with update_mappoint! and remove_mappoint_obs! on a tracked_ba.Record -> [(id, code, observer key-frame)] of the keypoints
    that pass :208-211, in ascending id order (the order of a slab)"""
    k, log = rec.cur, []
    frame = rec.kfs[k]
    for kpid in sorted(frame.px):
        mp = rec.mps.get(kpid)
        if mp is None or mp.is_3d:                               # :208-211 (a missing point: skipped, no clean-up)
            continue
        observers = sorted(mp.obs)
        if len(observers) < 2:
            log.append((kpid, FEW, -1))
            continue
        kfid = observers[0]
        if kfid == k:
            log.append((kpid, SELF, -1))
            continue
        okf = rec.kfs.get(kfid)
        if okf is None or kpid not in okf.px:
            log.append((kpid, ABSENT, kfid))
            continue
        rel, rel_inv, wob = observer_mats(okf.theta, frame.theta)
        r = pair(cam, rel, rel_inv, np.array(okf.px[kpid]), np.array(frame.px[kpid]), max_error, min_depth, min_parallax)
        if r["ok"]:
            mp.xyz = (wob @ r["left"])[:3]; mp.is_3d = True
            log.append((kpid, ACCEPTED, kfid))
        else:
            frame.px.pop(kpid); mp.obs.discard(k)
            log.append((kpid, REMOVED, kfid))
    return log
