"""The local-map match WITH the local-map history on the bounded key-frame map (test helper; never imported by the product): the model of
slam_kfmap_local_map_match once slam_kfmap_enable_local_map_history has been called.  State: an np_kfmap.Map, the descriptor dict of
np_kfmap_local_map.py and a History beside them.

History keeps, per ring slot, (kfid, set of ids): frame.local_map_ids of the key-frame that lives there.  local_map_match(m, D, H, ...) for the newest
key-frame K (slot r0 = K % R), in this order:

  0 purge    an id that does not own its table entry (ptag[id % mcap] != id) leaves every stored set; every size below counts what is left
  1 C        today's local map, np_kfmap_local_map.local_map_ids(m, D, cov) -- empty when no key-frame is covisible
  2 rule     map_manager.jl:350-354: P = the set stored for K (else empty); L = C if len(C) > 0.5 len(P) (in doubles), else P | C.  P is non-empty only
             when the match runs twice for one key-frame: the key-frame is a deepcopy of a current frame whose set is never written (map_manager.jl:174)
  3 chain    mapper.jl:274-286: if a key-frame is covisible and len(L) < max_local, the covisible key-frame with the SMALLEST id (the reference takes the
             first key of a Dict, its comment says "oldest"; Dicts are walked ascending here) gives its stored set: L |= it, if the slot's set is that
             key-frame's (a key-frame whose match was skipped gives nothing).  The reference's `kfid -= 1` walk has no counterpart: a covisible slot is
             a valid key-frame by construction
  4 store    hist[r0] = (K, L), whatever the status
  5 stage    the ids of L that pass the gates NOW (owned and not removed, 3-D, described, not observed by K), ascending: more than max_local -> status 2,
             none -> status 1, else the staging and the match of np_kfmap_local_map.local_map_match on that list (restated below: that function takes
             no list)

The call changes nothing else.  A merge does not touch the sets (prev_id stops owning its entry and goes at the next purge; new_id is gated out while K
observes it); reset() clears a stream's history.  Deviations from the reference: the stored sets hold ids that passed the gates when they were stored
(the reference stores raw ids and gates at match time: an id that fails a gate at K never passes one later, so only the sizes of steps 2 and 3 can
differ -- tests/test_kfmap_local_map_history_host.py compares with such a restatement), and the purge.

`mutant` breaks one rule, for the tests that show the scenes can tell: "nochain" (step 3 off), "newest" (the newest covisible key-frame for the oldest),
"rule" (step 2 inverted), "le" (`<=` for `<` in step 3's size test)."""
import math

import numpy as np

import np_kfmap as npk
import np_kfmap_local_map as nl
import np_local_map as nlm

MUTANTS = ("nochain", "newest", "rule", "le")


class History:
    def __init__(self, R):
        self.kf = [-1] * R
        self.sets = [set() for _ in range(R)]
        self.count = dict(replace=0, union=0, chained=0, purged=0)      # step 2's branches WITH a non-empty P; chains that added an id; ids purged

    def reset(self):
        self.kf = [-1] * len(self.kf)
        self.sets = [set() for _ in self.kf]

    def ids(self, m, kfid):
        """the stored set of key-frame kfid, ascending -- or None where the ring does not hold it or the slot's set is not its own"""
        b = kfid % m.R
        if kfid < 0 or m.tag[b] != kfid or self.kf[b] != kfid:
            return None
        return np.array(sorted(self.sets[b]), dtype=np.int64)

    def snapshot(self):
        return repr([(k, sorted(s)) for k, s in zip(self.kf, self.sets)])


def purge(m, H):
    for b in range(m.R):
        lost = {i for i in H.sets[b] if m.ptag[i % m.mcap] != i}
        H.count["purged"] += len(lost)
        H.sets[b] = H.sets[b] - lost


def gated(m, D, ids):
    """step 5's gates, ascending"""
    r0, out = m.cur % m.R, []
    for i in sorted(ids):
        e = m.entry(i)
        if e is None or not m.flags[e] & npk.F_3D or not D["has"][e] or m.mask[e] >> r0 & 1:
            continue
        out.append(int(i))
    return out


def _none():
    return dict(status=1, pairs=np.zeros((0, 2), dtype=np.int64), dist=np.zeros(0), lm_ids=np.zeros(0, dtype=np.int64), kp_ids=np.zeros(0, dtype=np.int64),
                proj_yx=np.zeros((0, 2)), best_kp=np.zeros(0, dtype=np.int32), best_dist=np.zeros(0), margin=math.inf, count={})


def staged_match(m, D, lm, cam, cell_size, params):
    """np_kfmap_local_map.local_map_match from its key-frame rows on, for the local map `lm` (ascending ids that pass the gates)"""
    none = _none()
    r0 = m.cur % m.R
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
        keypoints.append({"pixel": tuple(m.upx[r0, i]), "descriptors": D["rows"][e].reshape(1, 4).copy(), "observers": obs})
    if not lm or not keypoints:
        return none
    local_map = []
    for kpid in lm:
        e = kpid % m.mcap
        local_map.append({"position": m.xyz[e].copy(), "descriptors": D["rows"][e].reshape(1, 4).copy(), "observers": [row[b] for b in asc if m.mask[e] >> b & 1]})
    frame = {"Tcw": nl.tcw_of(m.theta[r0]), "cam": [float(v) for v in cam], "cell_size": int(cell_size), "nb_3d_kpts": nb3}
    keyframes = np.array([nl.tcw_of(m.theta[b]) for b in asc])
    out = nlm.do_local_map_matching(frame, keypoints, keyframes, local_map, params)
    took = np.flatnonzero(out["match"] >= 0)
    pairs = np.array([(kp_ids[j], lm[out["match"][j]]) for j in took], dtype=np.int64).reshape(-1, 2)
    dist = np.array([out["best_dist"][out["match"][j]] for j in took], dtype=np.float64)
    return dict(none, status=0, pairs=pairs, dist=dist, lm_ids=np.array(lm, dtype=np.int64), kp_ids=np.array(kp_ids, dtype=np.int64), proj_yx=out["proj_yx"],
                best_kp=out["best_kp"], best_dist=out["best_dist"], margin=out["margin"], count=out["count"])


def oldest(cov, tag):
    """the covisible slot of the smallest key-frame id (the "newest" mutant takes the largest)"""
    return min(cov, key=lambda b: tag[b])


def rule(C, P, has_cov, linked, max_local=None, mutant=None):
    """steps 2 and 3's decisions on the sets -> (replace, L before the chain, whether the chain runs)"""
    replace = float(len(C)) > 0.5 * float(len(P))
    if mutant == "rule":
        replace = not replace
    L = set(C) if replace else P | C
    bound = math.inf if max_local is None else max_local
    chain = bool(has_cov) and (len(L) <= bound if mutant == "le" else len(L) < bound) and mutant != "nochain" and bool(linked)
    return replace, L, chain


def local_map_match(m, D, H, cam, cell_size, params, max_local=None, mutant=None):
    """-> np_kfmap_local_map.local_map_match's dict plus C (step 1's ids), size (len(L) at step 3's test), chain (the ids step 3 added), branch
    ("replace" / "union" when P was non-empty, else None)"""
    purge(m, H)
    if m.cur < 0:
        return dict(_none(), C=[], size=0, chain=[], branch=None)
    K, r0 = int(m.cur), m.cur % m.R
    cov = nl.covisible_slots(m)
    C = set(nl.local_map_ids(m, D, cov)) if cov else set()
    P = set(H.sets[r0]) if H.kf[r0] == K else set()
    b = (max(cov, key=lambda b: m.tag[b]) if mutant == "newest" else oldest(cov, m.tag)) if cov else None
    replace, L, runs = rule(C, P, cov, b is not None and H.kf[b] == m.tag[b], max_local, mutant)
    branch = None
    if P:
        branch = "replace" if replace else "union"
        H.count[branch] += 1
    size, chain = len(L), set()
    if runs:
        chain = H.sets[b] - L
        L |= H.sets[b]
        H.count["chained"] += bool(chain)
    H.kf[r0], H.sets[r0] = K, set(L)
    lm = gated(m, D, L)
    extra = dict(C=sorted(C), size=size, chain=sorted(chain), branch=branch)
    if max_local is not None and len(lm) > max_local:
        return dict(staged_match(m, D, [], cam, cell_size, params), status=2, **extra)
    return dict(staged_match(m, D, lm, cam, cell_size, params), **extra)
