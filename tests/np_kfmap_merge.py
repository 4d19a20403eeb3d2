"""The merge of local-map matches on the bounded key-frame map (test helper; never imported by the product): the model of slam_kfmap_merge.

merge(m, pairs, lst) applies merge_mappoints (src/map_manager.jl:378-427) with update_keypoint! (src/frame.jl:290-307) to an np_kfmap.Map, pair by
pair; a pair is (prev_id, new_id) = (the key-frame's keypoint, the local-map point) as slam_kfmap_local_map_match returns it.

  validity    both ids own their table entries (not dead), prev_id != new_id, the new point is 3-D (`new_mp.is_3d || return`); else nothing changes
  observers   every slot of prev's observer mask with a valid tag whose slab holds a LIVE observation of prev_id: where the slab also holds a live
              observation of new_id nothing happens (`has_new && return false`: the prev observation stays, an orphan once prev is gone), else the
              observation's id becomes new_id -- pixel and live byte kept -- and the new point gains that observer bit
  order       a touched slab holds unique, ascending ids again: the renamed record moves to its place, a tombstone whose id equals an arriving new_id is
              dropped (so that a lower bound cannot land on it), other tombstones stay; a slab never grows
  points      prev's entry becomes F_DEAD (`pop!(m.map_points, prev_id)`, NOT remove_mappoint!: the observations that were not renamed stay); the new
              point gets F_OBS if the newest key-frame's slab was renamed to it; its position and F_BA are untouched
  live list   (lst is not None) a list that carries prev_id and not new_id: the slot takes new_id, is_3d = True, xyz = the new point's position in the
              map, every other field travels with it, the list is re-ordered so that ids ascend, its length is unchanged
  no list     (lst is None) prev's entry also gets F_GONE: later lists that still carry prev_id are not recorded as a fresh point

Deviations from the reference, the device call's too:
  covisibility  add_covisibility! has no counterpart: covisibility is derived from the observer masks
  descriptors   the map keeps ONE row per point: the new point keeps its own row and prev's row goes with prev; the reference appends prev's rows to
                keyframes_descriptors and mappoint_min_distance takes the minimum over all of them
  gone          the F_GONE mark of a merge without a list (the reference always has the current frame at hand)

The pairs of one call are one-to-one (no prev id twice, no new id twice, no id on both sides): check_pairs; anything else is an argument error.  Such
merges commute -- tests/test_kfmap_merge_host.py shows it against a sequential dict-and-set restatement applied in shuffled orders.

`mutant` breaks one rule, for the tests that show the scenes can tell: "unsorted" (rename without re-sorting), "has_new" (the has_new check ignored),
"flat" (merge into a 2-D new point), "tombstone" (the equal-id tombstone kept)."""
import numpy as np

import np_kfmap as npk

MUTANTS = ("unsorted", "has_new", "flat", "tombstone")


def check_pairs(pairs):
    """one-to-one: no prev id twice, no new id twice, no id on both sides of two pairs (a pair of one id is left to the validity rule)"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    prev, new = [int(v) for v in p[:, 0]], [int(v) for v in p[:, 1]]
    cross = any(prev[u] == new[t] for u in range(len(p)) for t in range(len(p)) if u != t)
    return len(set(prev)) == len(prev) and len(set(new)) == len(new) and not cross


def _find_live(ids, live, kpid, mutant):
    """the live observation of kpid in a slab (ids, live), or None; a binary search, as kfm_find_live (the mutants leave slabs unsorted: linear)"""
    if mutant is None:
        i = int(np.searchsorted(ids, kpid))
        return i if i < len(ids) and ids[i] == kpid and live[i] else None
    hit = [int(i) for i in np.flatnonzero(ids == kpid) if live[i]]
    return hit[0] if hit else None


def valid_pair(m, prev, new, mutant=None):
    ep, en = m.entry(prev), m.entry(new)
    return ep is not None and en is not None and prev != new and (bool(m.flags[en] & npk.F_3D) or mutant == "flat")


def merge(m, pairs, lst=None, with_list=None, mutant=None, log=None):
    """-> dict(applied, skipped, renamed, status, list): the counts slam_kfmap_merge reports and the list as the device leaves it (None without one).
    with_list: whether the call has a keypoint set (default: lst is not None).  Pairs that are not one-to-one: status 1, nothing changed.
    log (a dict): counts of what the call met -- has_new, tombstone, multi (slabs with more than one rename), front, back, flat_prev."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    with_list = lst is not None if with_list is None else with_list
    out_list = None if lst is None else {k: np.asarray(v).copy() for k, v in lst.items()}
    if not check_pairs(pairs):
        return dict(applied=0, skipped=0, renamed=0, status=1, list=out_list)
    log = {} if log is None else log
    for key in ("has_new", "tombstone", "multi", "front", "back", "flat_prev"):
        log.setdefault(key, 0)
    applied, skipped, renamed = [], 0, 0
    touched = {}                                                 # slot -> the new ids that arrive in its slab
    r0 = m.cur % m.R if m.cur >= 0 else -1
    # every look-up reads the slabs as the call found them (the device resolves all pairs before it rebuilds a slab); the pairs are disjoint, so
    # this is what pair-by-pair application gives (the restatement test)
    slab = [(m.ids[b, :int(m.n[b])].copy(), m.live[b, :int(m.n[b])].copy()) for b in range(m.R)]
    for prev, new in ((int(a), int(b)) for a, b in pairs):
        if not valid_pair(m, prev, new, mutant):
            skipped += 1
            continue
        ep, en = prev % m.mcap, new % m.mcap
        log["flat_prev"] += not m.flags[ep] & npk.F_3D
        for b in range(m.R):
            if not (m.mask[ep] >> b & 1) or m.tag[b] < 0:
                continue
            i = _find_live(*slab[b], prev, mutant)
            if i is None:
                continue
            if _find_live(*slab[b], new, mutant) is not None and mutant != "has_new":
                log["has_new"] += 1
                continue
            m.ids[b, i] = new
            m.mask[en] |= 1 << b
            touched.setdefault(b, set()).add(new)
            renamed += 1
            if b == r0:
                m.flags[en] |= npk.F_OBS
        m.mask[ep] = 0
        m.flags[ep] = npk.F_DEAD | (m.flags[ep] & npk.F_GONE) | (0 if with_list else npk.F_GONE)
        applied.append((prev, new))
    for b, arrived in touched.items():                                 # the order invariant, slab by slab
        n = int(m.n[b])
        ids, upx, live = m.ids[b, :n].copy(), m.upx[b, :n].copy(), m.live[b, :n].copy()
        log["multi"] += len(arrived) > 1
        keep = np.array([bool(live[i]) or int(ids[i]) not in arrived for i in range(n)], dtype=bool)
        log["tombstone"] += int((~keep).sum())
        if mutant == "tombstone":
            keep[:] = True
        if mutant == "unsorted":
            order = np.flatnonzero(keep)
        else:
            order = np.flatnonzero(keep)[np.argsort(ids[keep], kind="stable")]
            moved = [int(np.flatnonzero(order == i)[0]) for i in range(n) if live[i] and int(ids[i]) in arrived and keep[i]]
            log["front"] += 0 in moved; log["back"] += len(order) - 1 in moved
        k2 = len(order)
        m.ids[b, :k2] = ids[order]; m.upx[b, :k2] = upx[order]; m.live[b, :k2] = live[order]
        m.n[b] = k2
    if out_list is not None:
        ids = out_list["ids"].astype(np.int64)
        have = set(int(i) for i in ids)
        for prev, new in applied:
            if prev in have and new not in have:
                j = int(np.flatnonzero(ids == prev)[0])
                ids[j] = new
                out_list["is_3d"][j] = True
                out_list["xyz"][j] = m.xyz[new % m.mcap]
        order = np.arange(len(ids)) if mutant == "unsorted" else np.argsort(ids, kind="stable")
        out_list["ids"] = ids
        out_list = {k: v[order] for k, v in out_list.items()}
    return dict(applied=len(applied), skipped=skipped, renamed=renamed, status=0, list=out_list)


# ---- the sequential restatement on tests/tracked_ba.py's unbounded Record: dicts and sets only -----------------------------------------------------------
def restated_merge(rec, prev_id, new_id, with_list=True):
    """merge_mappoints (map_manager.jl:378-427) for one pair on a tracked_ba.Record; -> the number of key-frames whose keypoint was renamed, or None
    where the reference returns early"""
    prev_mp = rec.mps.get(prev_id)
    if prev_mp is None:
        return None
    new_mp = rec.mps.get(new_id)
    if new_mp is None or prev_id == new_id:
        return None
    if not new_mp.is_3d:
        return None
    n = 0
    for o in sorted(prev_mp.obs):
        kf = rec.kfs.get(o)
        if kf is None:
            continue
        if new_id in kf.px:                                      # update_keypoint!: has_new && return false
            continue
        if prev_id not in kf.px:
            continue
        kf.px[new_id] = kf.px.pop(prev_id)
        new_mp.obs.add(o)                                        # add_keyframe_observation!
        if o == rec.cur:
            new_mp.observed = True
        n += 1
    rec.mps.pop(prev_id)
    if not with_list:
        rec.gone.add(prev_id)
    return n


def snapshot(m):
    """the whole state of a map as comparable bytes: the ring (tags, lengths, the slabs up to their lengths) and the table"""
    ring = [(int(m.tag[b]), int(m.n[b]), m.ids[b, :int(m.n[b])].tobytes(), m.upx[b, :int(m.n[b])].tobytes(), m.live[b, :int(m.n[b])].tobytes()) for b in range(m.R)]
    return repr((ring, m.ptag.tobytes(), m.flags.tobytes(), tuple(int(v) for v in m.mask), m.xyz.tobytes(), m.cur))


def sorted_unique(m):
    """the order invariant: every slab's ids ascend strictly"""
    return all(np.all(np.diff(m.ids[b, :int(m.n[b])]) > 0) for b in range(m.R))
