"""The local-map match on the bounded key-frame map (test helper; never imported by the product): the model of slam_kfmap_local_map_match.

State: an np_kfmap.Map and a descriptor dict {"has": (mcap,) bool, "rows": (mcap, 4) uint64} kept beside it by add_keyframe / add_descriptors
below (the row of point `id` at entry id % mcap, owned under the table's rule: a point that is replaced, or recorded anew after its removal, loses it).

local_map_match(m, D, cam, cell_size, params) restates update_frame_covisibility! (src/map_manager.jl:302-355) on the bounded map -- the covisible
key-frames, then the local map with the gates of do_local_map_matching (src/mapper.jl:338-341) -- builds `frame`, `keypoints`, `keyframes` and
`local_map` in the form np_local_map.do_local_map_matching takes, calls it, and returns the pairs, the staged order and the margin.  The stated
deviations of the device call are the model's too: frame.local_map_ids is not kept between key-frames (neither :350-354 nor mapper.jl:274-286), no
remove_mappoint_obs! clean-ups, no merges, undistorted pixels (the callers use cameras without distortion), sets walked ascending by id.

`mutant` switches one rule off, for the tests that show the scenes can tell: "own" (the frame's own points not excluded), "descending" (local map in
descending order), "lt" (`<` for `<=` in the reverse selection, mapper.jl:375), "dead" (dead observations counted)."""
import math

import numpy as np

import np_kfmap as npk
import np_local_map as nlm


def tcw_of(theta):
    """angles_to_pose (csrc/pose_records.hpp): RotZYX(theta1..3) and the translation as a 4 x 4; products associate left to right"""
    s1, c1, s2, c2, s3, c3 = (math.sin(theta[0]), math.cos(theta[0]), math.sin(theta[1]), math.cos(theta[1]), math.sin(theta[2]), math.cos(theta[2]))
    T = np.eye(4)
    T[:3, :3] = [[c1 * c2, c1 * s2 * s3 - s1 * c3, c1 * s2 * c3 + s1 * s3], [s1 * c2, s1 * s2 * s3 + c1 * c3, s1 * s2 * c3 - c1 * s3], [-s2, c2 * s3, c2 * c3]]
    T[:3, 3] = theta[3:6]
    return T


def new_descriptors(m):
    return {"has": np.zeros(m.mcap, dtype=bool), "rows": np.zeros((m.mcap, 4), dtype=np.uint64)}


def add_keyframe(m, D, kfid, Tcw, lst):
    """np_kfmap.add_keyframe, and the descriptor of every entry that takes a new point goes"""
    before, flags = m.ptag.copy(), m.flags.copy()
    npk.add_keyframe(m, kfid, Tcw, lst)
    for i in np.asarray(lst["ids"], dtype=np.int64):
        e = int(i) % m.mcap
        if m.ptag[e] != i or (before[e] == i and flags[e] & npk.F_GONE):         # an orphan, or an id the frame has lost: not recorded
            continue
        if before[e] != i or flags[e] & npk.F_DEAD:
            D["has"][e] = False


def add_descriptors(m, D, first_id, rows):
    """slam_kfmap_add_descriptors for one stream: row j belongs to id first_id + j, stored where the entry carries that id"""
    for j, row in enumerate(np.asarray(rows, dtype=np.uint64).reshape(-1, 4)):
        e = (int(first_id) + j) % m.mcap
        if m.ptag[e] == int(first_id) + j:
            D["rows"][e] = row; D["has"][e] = True


def covisible_slots(m):
    """update_frame_covisibility! :303-326 on the bounded map -> {slot: score} of the other valid key-frames that share a live, owned point with the newest"""
    r0, cov = m.cur % m.R, {}
    for i in range(int(m.n[r0])):
        if not m.live[r0, i]:
            continue
        e = m.entry(m.ids[r0, i])
        if e is None:                                                           # :310-314 (without the clean-up)
            continue
        for b in range(m.R):
            if b != r0 and m.mask[e] >> b & 1 and m.tag[b] >= 0:                # :318-325; :334 `kfid in frames_map`
                cov[b] = cov.get(b, 0) + 1
    return cov


def local_map_ids(m, D, cov, mutant=None):
    """:333-343 with the gates of mapper.jl:338-341, ascending by id"""
    r0, ids = m.cur % m.R, set()
    for b in cov:
        for i in range(int(m.n[b])):
            if not m.live[b, i] and mutant != "dead":
                continue
            kpid = int(m.ids[b, i])
            e = m.entry(kpid)
            if e is None or not m.flags[e] & npk.F_3D or not D["has"][e]:      # get_3d_keypoints; mapper.jl:339-341
                continue
            if m.mask[e] >> r0 & 1 and mutant != "own":                        # :341 / mapper.jl:338: not the frame's own
                continue
            ids.add(kpid)
    return sorted(ids, reverse=mutant == "descending")


def local_map_match(m, D, cam, cell_size, params, max_local=None, mutant=None):
    """-> dict(status, pairs (n, 2) int64, dist (n,), lm_ids, kp_ids, proj_yx, best_kp, best_dist, margin, count, problem)"""
    none = dict(status=1, pairs=np.zeros((0, 2), dtype=np.int64), dist=np.zeros(0), lm_ids=np.zeros(0, dtype=np.int64), kp_ids=np.zeros(0, dtype=np.int64),
                proj_yx=np.zeros((0, 2)), best_kp=np.zeros(0, dtype=np.int32), best_dist=np.zeros(0), margin=math.inf, count={}, problem=None)
    if m.cur < 0:
        return none
    r0 = m.cur % m.R
    cov = covisible_slots(m)
    if not cov:
        return none
    lm = local_map_ids(m, D, cov, mutant)
    if max_local is not None and len(lm) > max_local:
        return dict(none, status=2)
    asc = sorted((b for b in range(m.R) if m.tag[b] >= 0), key=lambda b: m.tag[b])          # key-frame rows: the valid slots, ascending by id
    row = {b: k for k, b in enumerate(asc)}
    kp_ids, keypoints, nb3 = [], [], 0
    for i in range(int(m.n[r0])):
        if not m.live[r0, i]:
            continue
        kpid = int(m.ids[r0, i])
        e = m.entry(kpid)
        if e is None:
            continue
        nb3 += bool(m.flags[e] & npk.F_3D)
        if not D["has"][e]:
            continue
        obs = []
        for b in asc:
            if m.mask[e] >> b & 1:
                j = m.find_live(b, kpid)
                if j is not None:                                               # mapper.jl:429-434: a missing observation is skipped
                    obs.append((row[b], tuple(m.upx[b, j])))
        kp_ids.append(kpid)
        keypoints.append({"pixel": tuple(m.upx[r0, i]), "descriptors": D["rows"][e].reshape(1, 4).copy(), "observers": obs})
    if not lm or not keypoints:
        return none
    local_map = []
    for kpid in lm:
        e = kpid % m.mcap
        local_map.append({"position": m.xyz[e].copy(), "descriptors": D["rows"][e].reshape(1, 4).copy(), "observers": [row[b] for b in asc if m.mask[e] >> b & 1]})
    frame = {"Tcw": tcw_of(m.theta[r0]), "cam": [float(v) for v in cam], "cell_size": int(cell_size), "nb_3d_kpts": nb3}
    keyframes = np.array([tcw_of(m.theta[b]) for b in asc])
    out = nlm.do_local_map_matching(frame, keypoints, keyframes, local_map, params)
    match = out["match"]
    if mutant == "lt":                                                          # the reverse selection with `<`: among equal distances the FIRST point wins
        match = np.full(len(keypoints), -1, dtype=np.int32)
        for j in range(len(keypoints)):
            best = 1e6
            for k in np.flatnonzero(out["best_kp"] == j):
                if out["best_dist"][k] < best:
                    best, match[j] = out["best_dist"][k], k
    took = np.flatnonzero(match >= 0)
    pairs = np.array([(kp_ids[j], lm[match[j]]) for j in took], dtype=np.int64).reshape(-1, 2)
    dist = np.array([out["best_dist"][match[j]] for j in took], dtype=np.float64)
    return dict(status=0, pairs=pairs, dist=dist, lm_ids=np.array(lm, dtype=np.int64), kp_ids=np.array(kp_ids, dtype=np.int64), proj_yx=out["proj_yx"],
                best_kp=out["best_kp"], best_dist=out["best_dist"], margin=out["margin"], count=out["count"],
                problem=(frame, keypoints, keyframes, local_map, params))
