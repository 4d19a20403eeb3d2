"""map_filtering! (src/estimator.jl:358-406) and the remove_keyframe! it calls (src/map_manager.jl:184-209) on the bounded key-frame map
(test helper; never imported by the product): two routines over np_kfmap.Map, the model slam_kfmap_filter / slam_kfmap_remove_keyframe are
held to, and their unbounded twins over tracked_ba.Record's dicts.  While kf < R and ids < mcap the two agree state for state
(tests/test_kfmap_filter_host.py).

What the bounded model fixes where the reference leaves it open, or drops:
  * candidates: the covisibility map of the newest key-frame as the gather's first pass forms it -- every other slot with a valid tag that shares
    at least one live, owned point with the newest slab (2-D points count) -- walked ASCENDING by key-frame id (the reference walks a Dict);
  * `kfid == 0 && break` is kept literally: while key-frame 0 is covisible with the newest key-frame nothing is filtered;
  * `estimator.new_kf_available && break` has no counterpart (lock-stepped streams never race);
  * kf.nb_3d_kpts and n_total are ONE count: the candidate's live observations whose point's entry carries F_3D.  (The reference keeps
    nb_3d_kpts as a counter of the frame and n_total as a walk over its 3-D keypoints; the map keeps is_3d per point only.)  An orphan is
    skipped and left as it is;
  * n_good counts those points with more than four observers, evaluated after the removals this same call has already made;
  * the ratio test is one IEEE double division: 0 / 0 is NaN and keeps the key-frame;
  * remove_keyframe makes no is_bad evaluation (the reference makes none; the next gather demotes what became bad), leaves the live lists
    alone, and has no remove_covisible_kf! (covisibility is derived from the masks on demand)."""
import numpy as np

import kfmap_scripts as scr
import np_kfmap as km

FIRST_KFID = 20                         # the reference's literal (estimator.jl:360)

# The scripted case of both test files: S = 4 streams of 14 key-frames, cap 100, mcap 1024, min_cov_score 8, first_kfid 6; after each key-frame
# gather -> update (scr.refined / scr.outlier_pattern) -> filter.  The fourth stream's ratio is 1.0: its filter never acts.
CAP, MCAP, MINC, FIRST = 100, 1024, 8, 6
SIZES = (60, 64, 70, 65, 80, 100, 90, 30, 64, 65, 100, 12, 80, 70)
STREAMS = (dict(seed=3, p_drop=0.25, p_long=0.25, ratio=0.5), dict(seed=5, p_drop=0.1, p_long=0.6, ratio=0.6),
           dict(seed=8, p_drop=0.05, p_long=0.8, ratio=0.7), dict(seed=11, p_drop=0.1, p_long=0.6, ratio=1.0))


def frames(cfg, sizes=SIZES):
    return scr.make_stream(cfg["seed"], sizes, p_drop=cfg["p_drop"], p_long=cfg["p_long"])


# ---- the bounded model -------------------------------------------------------------------------------------------------------------------
def remove_keyframe(m, kfid):
    b = m.slot(kfid)
    if b is None:
        return
    if kfid == m.cur:
        raise ValueError("the newest key-frame cannot be removed")
    for i in range(int(m.n[b])):                                 # remove_kf_observation!, as add_keyframe's forgetting
        if m.live[b, i]:
            e = int(m.ids[b, i]) % m.mcap
            if m.ptag[e] == m.ids[b, i]:
                m.mask[e] &= ~(1 << b)
    m.tag[b] = -1; m.n[b] = 0


def ascending_ids(tag, slots):
    """the key-frame ids of `slots`, ascending"""
    return sorted(int(tag[b]) for b in slots)


def walked(cands, cur):
    """the candidates the walk evaluates -> (their ids, whether key-frame 0 ended the walk): an id >= the newest is passed over"""
    out = []
    for kfid in cands:
        if kfid == 0:
            return out, True
        if kfid < cur:
            out.append(kfid)
    return out, False


def covisible(m):
    """the slots of the key-frames covisible with the newest one"""
    r0 = m.cur % m.R
    cov = set()
    for i in range(int(m.n[r0])):
        if not m.live[r0, i]:
            continue
        e = m.entry(m.ids[r0, i])
        if e is None:
            continue
        cov |= {b for b in range(m.R) if b != r0 and m.mask[e] >> b & 1 and m.tag[b] >= 0}
    return cov


def candidates(m):
    """the covisible key-frames of the newest one, ascending by id"""
    return ascending_ids(m.tag, covisible(m))


def _decide(n_total, n_good, filtering_ratio, min_cov_score):
    if n_total < min_cov_score // 2:
        return "few"
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.float64(n_good) / np.float64(n_total)
    return "ratio" if ratio > filtering_ratio else "keep"


def filter_map(m, filtering_ratio, min_cov_score, first_kfid=FIRST_KFID):
    """-> [(kfid, exit, n_total, n_good)], exit in break / keep / few / ratio"""
    log = []
    if filtering_ratio >= 1 or m.cur < first_kfid:
        return log
    kfids, broke = walked(candidates(m), m.cur)
    if broke:                                                    # (key-frame 0 is the smallest id: nothing was walked before it)
        log.append((0, "break", 0, 0))
    for kfid in kfids:
        b = m.slot(kfid)
        n_total = n_good = 0
        for i in range(int(m.n[b])):
            if not m.live[b, i]:
                continue
            e = m.entry(m.ids[b, i])
            if e is None or not m.flags[e] & km.F_3D:
                continue
            n_total += 1
            n_good += len(m.observers(e)) > 4
        ex = _decide(n_total, n_good, filtering_ratio, min_cov_score)
        if ex != "keep":
            remove_keyframe(m, kfid)
        log.append((kfid, ex, n_total, n_good))
    return log


# ---- the unbounded twin over tracked_ba.Record ---------------------------------------------------------------------------------------------
def remove_keyframe_record(rec, kfid):
    kf = rec.kfs.get(kfid)
    if kf is None:
        return
    if kfid == rec.cur:
        raise ValueError("the newest key-frame cannot be removed")
    for kp in kf.px:
        mp = rec.mps.get(kp)
        if mp is not None:
            mp.obs.discard(kfid)
    del rec.kfs[kfid]


def filter_record(rec, filtering_ratio, min_cov_score, first_kfid=FIRST_KFID):
    import tracked_ba as tb
    log = []
    if filtering_ratio >= 1 or rec.cur < first_kfid:
        return log
    for kfid in sorted(k for k in tb.covisibility(rec, rec.cur) if k in rec.kfs):
        if kfid == 0:
            log.append((0, "break", 0, 0))
            break
        if kfid >= rec.cur:
            continue
        n_total = n_good = 0
        for kp in rec.kfs[kfid].px:
            mp = rec.mps.get(kp)
            if mp is None or not mp.is_3d:
                continue
            n_total += 1
            n_good += len(mp.obs) > 4
        ex = _decide(n_total, n_good, filtering_ratio, min_cov_score)
        if ex != "keep":
            remove_keyframe_record(rec, kfid)
        log.append((kfid, ex, n_total, n_good))
    return log


def removed_mask(log, R):
    """the word slam_kfmap_filter returns for a stream: bit k % R per removed key-frame k"""
    w = 0
    for kfid, ex, _, _ in log:
        if ex in ("few", "ratio"):
            w |= 1 << (kfid % R)
    return w
