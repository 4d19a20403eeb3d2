"""Descriptor rows on the bounded key-frame map (test helper; never imported by the product): the model of slam_kfmap_enable_descriptor_rows --
a map point keeps one 256-bit row per key-frame id, the reference's keyframes_descriptors (src/map_point.jl:15), at most D of them.

State: an np_kfmap.Map and a descriptor dict as np_kfmap_local_map keeps it ("has", "rows"), with three more entries: "krows" (per table entry a
dict key-frame id -> (4,) uint64 row), "max_rows" (D) and "dropped" (rows dropped by the bound so far).  "has" is the reference's "mp.descriptor
is not empty"; "rows" stays what add_descriptors wrote (the reference's most representative descriptor is not modelled).

Every operation of the base models runs through upkeep(): after it,
  * an entry whose owner changed (another id, or a removed id recorded anew) has no rows;
  * every observer bit of an unchanged owner that went 1 -> 0 drops the row keyed by that slot's key-frame (remove_kf_observation!,
    map_point.jl:88-122: pop!(keyframes_descriptors, kfid));
  * an unchanged owner that lost a bit and has no valid observer left (no bit whose slot holds a key-frame) has no rows and is no longer described
    (:92-96).
add_keyframe() runs the forgetting of a reused ring slot as a step of its own before the recording: a point seen by key-frame k - R and by k keeps
its bit across the call, but the old key-frame's row goes (the ring's reuse counts as remove_keyframe!).
add_descriptors() also puts the row under the key of the newest key-frame (add_mappoint!'s current_keyframe_id); merge() copies prev's rows into
the surviving point, an equal key keeps the survivor's (map_manager.jl:410-412, add_descriptor! map_point.jl:124-131).
The bound: put() into a point that holds D rows keeps the D rows with the LARGEST keys among the D + 1 and counts one dropped row -- whatever the
order of arrival, the D largest keys of a union stay.
local_map_match() is np_kfmap_local_map.local_map_match with every row of a point, ascending by key, as its descriptors: the distance of a pair is
the minimum over all pairs of rows (mappoint_min_distance, map_point.jl:165-174); a described point without a row has none and is never chosen.

`mutant` breaks one rule, for the tests that show the scenes can tell: "no_move" (prev's rows not moved on merge), "overwrite" (no equal-key skip:
prev's row replaces the survivor's), "keep_row" (the row not dropped when its key-frame's observation goes), "keep_last" (rows not cleared when
the last observer goes)."""
import math

import numpy as np

import np_kfmap as npk
import np_kfmap_filter as npf
import np_kfmap_local_map as nl
import np_kfmap_merge as nm
import np_local_map as nlm

MUTANTS = ("no_move", "overwrite", "keep_row", "keep_last")


def new_descriptors(m, max_rows):
    D = nl.new_descriptors(m)
    D.update(krows=[dict() for _ in range(m.mcap)], max_rows=int(max_rows), dropped=0)
    return D


# ---- the row set of one point: a dict key-frame id -> row, bounded ---------------------------------------------------------------------------------------
def put(rows, kfid, row, max_rows, overwrite=False):
    """add_descriptor! under the bound -> rows dropped (0 or 1)"""
    if kfid in rows and not overwrite:
        return 0
    rows[int(kfid)] = np.array(row, dtype=np.uint64)
    if len(rows) <= max_rows:
        return 0
    del rows[min(rows)]
    return 1


def union(rows, prev_rows, max_rows, overwrite=False):
    """merge_mappoints' copy (map_manager.jl:410-412) under the bound -> rows dropped"""
    n = len(set(rows) | set(prev_rows))
    for k in sorted(prev_rows):
        put(rows, k, prev_rows[k], max_rows, overwrite)
    return max(n - max_rows, 0)                                  # the keys of the union beyond D, whatever the order they arrived in


def in_order(rows):
    """-> (keys (k,) int32 ascending, rows (k, 4) uint64 in that order)"""
    ks = sorted(rows)
    return np.array(ks, dtype=np.int32), np.array([rows[k] for k in ks], dtype=np.uint64).reshape(-1, 4)


# ---- the upkeep ------------------------------------------------------------------------------------------------------------------------------------------
def snapshot(m):
    return m.ptag.copy(), list(m.mask), m.tag.copy(), m.flags.copy()


def _valid(m, e):
    return any(m.mask[e] >> b & 1 and m.tag[b] >= 0 for b in range(m.R))


def upkeep(m, D, snap, mutant=None):
    ptag, mask, tag, flags = snap
    for e in range(m.mcap):
        if m.ptag[e] != ptag[e] or (flags[e] & npk.F_DEAD and not m.flags[e] & npk.F_DEAD):        # a new owner (base model: "has" is cleared there)
            D["krows"][e] = {}
            continue
        lost = mask[e] & ~m.mask[e]
        if not lost:
            continue
        if mutant != "keep_row":
            for b in range(m.R):
                if lost >> b & 1 and tag[b] >= 0:
                    D["krows"][e].pop(int(tag[b]), None)
        if not _valid(m, e) and mutant != "keep_last":
            D["krows"][e] = {}; D["has"][e] = False


def through(fn):
    """fn(m, ...) of a base model as an operation on (m, D): the rows follow what it did to owners and observers"""
    def op(m, D, *a, mutant=None, **kw):
        snap = snapshot(m)
        out = fn(m, *a, **kw)
        upkeep(m, D, snap, mutant)
        return out
    return op


gather = through(npk.gather)
update = through(npk.update)
filter_map = through(npf.filter_map)
remove_keyframe = through(npf.remove_keyframe)


def add_keyframe(m, D, kfid, Tcw, lst, mutant=None):
    r = kfid % m.R
    if m.tag[r] >= 0 and m.tag[r] != kfid:                       # the forgetting, a step of its own (what np_kfmap.add_keyframe does first)
        snap = snapshot(m)
        for i in range(int(m.n[r])):
            if m.live[r, i]:
                e = int(m.ids[r, i]) % m.mcap
                if m.ptag[e] == m.ids[r, i]:
                    m.mask[e] &= ~(1 << r)
        upkeep(m, D, snap, mutant)
    snap = snapshot(m)
    nl.add_keyframe(m, D, kfid, Tcw, lst)
    upkeep(m, D, snap, mutant)


def add_descriptors(m, D, first_id, rows):
    """slam_kfmap_add_descriptors with rows: the row also goes under the key of the stream's newest key-frame"""
    nl.add_descriptors(m, D, first_id, rows)
    for j, row in enumerate(np.asarray(rows, dtype=np.uint64).reshape(-1, 4)):
        e = (int(first_id) + j) % m.mcap
        if m.ptag[e] == int(first_id) + j:
            D["dropped"] += put(D["krows"][e], m.cur, row, D["max_rows"])


def merge(m, D, pairs, lst=None, with_list=None, mutant=None, log=None):
    """np_kfmap_merge.merge, and every applied pair's new point takes prev's rows"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    applied = [(int(a), int(b)) for a, b in pairs if nm.valid_pair(m, int(a), int(b))] if nm.check_pairs(pairs) else []
    moved = {b: dict(D["krows"][a % m.mcap]) for a, b in applied}
    snap = snapshot(m)
    out = nm.merge(m, pairs, lst, with_list=with_list, log=log)
    upkeep(m, D, snap, mutant)                                   # prev has lost every observer: its rows are gone
    for new, prev_rows in moved.items():
        if mutant == "no_move":
            continue
        if prev_rows:
            D["has"][new % m.mcap] = True                        # add_descriptor! into an empty set: the point is described from then on
        D["dropped"] += union(D["krows"][new % m.mcap], prev_rows, D["max_rows"], overwrite=mutant == "overwrite")
    return out


def descriptor_rows(m, D):
    """what KeyframeMap.descriptor_rows returns for the stream"""
    es = sorted((int(m.ptag[e]), e) for e in range(m.mcap) if m.ptag[e] >= 0 and not m.flags[e] & npk.F_DEAD)
    got = [in_order(D["krows"][e]) for _, e in es]
    return dict(ids=np.array([i for i, _ in es], dtype=np.int64), described=np.array([bool(D["has"][e]) for _, e in es], dtype=bool),
                keys=[g[0] for g in got], rows=[g[1] for g in got], dropped=int(D["dropped"]))


def same_rows(a, b):
    """two descriptor_rows() results, array for array"""
    return (np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["described"], b["described"]) and a["dropped"] == b["dropped"] and
            len(a["keys"]) == len(b["keys"]) and all(np.array_equal(x, y) for x, y in zip(a["keys"], b["keys"])) and
            all(np.array_equal(x, y) for x, y in zip(a["rows"], b["rows"])))


# ---- the match -------------------------------------------------------------------------------------------------------------------------------------------
def local_map_match(m, D, cam, cell_size, params, max_local=None, one_row=False):
    """np_kfmap_local_map.local_map_match with the rows of every point as its descriptors (one_row: the single row "rows", the map without rows,
    on the same state) -> the same dict, plus lm_rows / kp_rows: the row count of every staged record"""
    none = dict(status=1, pairs=np.zeros((0, 2), dtype=np.int64), dist=np.zeros(0), lm_ids=np.zeros(0, dtype=np.int64), kp_ids=np.zeros(0, dtype=np.int64),
                proj_yx=np.zeros((0, 2)), best_kp=np.zeros(0, dtype=np.int32), best_dist=np.zeros(0), margin=math.inf, count={}, problem=None,
                lm_rows=np.zeros(0, dtype=np.int64), kp_rows=np.zeros(0, dtype=np.int64))
    desc = (lambda e: D["rows"][e].reshape(1, 4).copy()) if one_row else (lambda e: in_order(D["krows"][e])[1])
    if m.cur < 0:
        return none
    r0 = m.cur % m.R
    cov = nl.covisible_slots(m)
    if not cov:
        return none
    lm = nl.local_map_ids(m, D, cov)
    if max_local is not None and len(lm) > max_local:
        return dict(none, status=2)
    asc = sorted((b for b in range(m.R) if m.tag[b] >= 0), key=lambda b: m.tag[b])
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
                if j is not None:
                    obs.append((row[b], tuple(m.upx[b, j])))
        kp_ids.append(kpid)
        keypoints.append({"pixel": tuple(m.upx[r0, i]), "descriptors": desc(e), "observers": obs})
    if not lm or not keypoints:
        return none
    local_map = []
    for kpid in lm:
        e = kpid % m.mcap
        local_map.append({"position": m.xyz[e].copy(), "descriptors": desc(e), "observers": [row[b] for b in asc if m.mask[e] >> b & 1]})
    frame = {"Tcw": nl.tcw_of(m.theta[r0]), "cam": [float(v) for v in cam], "cell_size": int(cell_size), "nb_3d_kpts": nb3}
    keyframes = np.array([nl.tcw_of(m.theta[b]) for b in asc])
    out = nlm.do_local_map_matching(frame, keypoints, keyframes, local_map, params)
    match = out["match"]
    took = np.flatnonzero(match >= 0)
    pairs = np.array([(kp_ids[j], lm[match[j]]) for j in took], dtype=np.int64).reshape(-1, 2)
    dist = np.array([out["best_dist"][match[j]] for j in took], dtype=np.float64)
    return dict(status=0, pairs=pairs, dist=dist, lm_ids=np.array(lm, dtype=np.int64), kp_ids=np.array(kp_ids, dtype=np.int64), proj_yx=out["proj_yx"],
                best_kp=out["best_kp"], best_dist=out["best_dist"], margin=out["margin"], count=out["count"],
                problem=(frame, keypoints, keyframes, local_map, params),
                lm_rows=np.array([len(p["descriptors"]) for p in local_map], dtype=np.int64),
                kp_rows=np.array([len(k["descriptors"]) for k in keypoints], dtype=np.int64))
