"""Scripted sequences for the merge on the key-frame map (test helper): the scenes of tests/kfmap_lmm_scripts.py (S = 3, cap 64, R = 4, mcap = 128), whose
copies and twins produce real pairs, driven through add_keyframe -> add_descriptors -> local_map_match -> merge at every key-frame, in two modes:

  "follow"   the merge has the live lists (ks): later scripted lists follow the renames -- every id mapped through the merges so far and the list
             re-sorted, as a live front end would produce them;
  "stale"    the merge has no list (ks = NULL): later lists still carry the prev ids, which are marked gone and dead -- recorded as tombstones, never as
             fresh points.

The match never pairs two ids that share a slab (a copy is born after its original has left the lists), so behind key-frame HAND_AT a second merge with
pairs picked from the model's state (hand_pairs) brings the two kinds the scenes cannot produce: a slab that holds both ids alive (the has_new skip,
which leaves an orphan) and a slab that holds prev alive and a tombstone of new (the equal-id tombstone, dropped).

hand_scene(): a hand-built sequence at cap = 300 (R = 4, mcap = 1024, five key-frames), so that a slab spans two 256-record chunks and renames cross
the chunk edge; HAND_PAIRS names what each of its pairs is there for."""
import numpy as np

import kfmap_lmm_scripts as ls
import kfmap_scripts as scr
import np_kfmap as npk
import np_kfmap_local_map as nl
import np_kfmap_merge as nm

MODES = ("follow", "stale")
HAND_AT = 5                              # the ring then holds key-frames 2 .. 5, with the tombstones of the updates behind key-frames 3 and 4
S = ls.S


def hand_pairs(m, avoid=()):
    """-> ([(prev, new)], kinds): one pair for a slab that holds prev alive and a tombstone of new ("tombstone"), one for a slab that holds both alive
    while another holds prev alone ("has_new"), where the state has them; no id twice, none of `avoid`"""
    used, pairs, kinds = set(int(i) for i in avoid), [], []
    slots = [b for b in range(m.R) if m.tag[b] >= 0]
    live = {b: {int(m.ids[b, i]) for i in range(int(m.n[b])) if m.live[b, i]} for b in slots}
    ok = lambda i: m.entry(i) is not None and i not in used
    for b in slots:                                              # the equal-id tombstone
        if "tombstone" in kinds:
            break
        for i in range(int(m.n[b])):
            t = int(m.ids[b, i])
            if m.live[b, i] or not ok(t) or not m.flags[t % m.mcap] & npk.F_3D:
                continue
            prev = [p for p in sorted(live[b]) if ok(p) and p != t and (m.mask[p % m.mcap] >> b & 1)]
            if prev:
                pairs.append((prev[0], t)); kinds.append("tombstone"); used |= {prev[0], t}
                break
    for b in slots:                                              # has_new, with a rename elsewhere
        if "has_new" in kinds:
            break
        for new in sorted(live[b]):
            if not ok(new) or not m.flags[new % m.mcap] & npk.F_3D:
                continue
            prev = [p for p in sorted(live[b]) if ok(p) and p != new and (m.mask[p % m.mcap] >> b & 1)
                    and any(c != b and p in live[c] and new not in live[c] and (m.mask[p % m.mcap] >> c & 1) for c in slots)]
            if prev:
                pairs.append((prev[0], new)); kinds.append("has_new"); used |= {prev[0], new}
                break
    return pairs, kinds


class MergeRun(ls.ModelRun):
    """ModelRun with the merge behind every match.  lists[s]: stream s's live list as the model has it (what KeypointSet.download must return);
    ren[s]: prev id -> new id of every pair applied so far; log[s]: np_kfmap_merge's counts of what the merges met; counts: the last merge's (S, 4)."""

    def __init__(self, mode, **kw):
        assert mode in MODES
        frames, descs = ls.scenes()
        super().__init__(frames, descs, **kw)
        self.mode = mode
        self.lists = [None] * self.n
        self.ren = [dict() for _ in range(self.n)]
        self.log = [dict() for _ in range(self.n)]
        self.counts = np.zeros((self.n, 4), dtype=np.int32)

    def mapped(self, s, f):
        """the scripted list as a front end that followed the renames would hand it over"""
        if self.mode != "follow" or not self.ren[s]:
            return f
        ids, have = [], set(int(i) for i in f["ids"])
        for i in (int(i) for i in f["ids"]):
            j = i
            while j in self.ren[s]:
                j = self.ren[s][j]
            if j != i and j in have:                             # the list carries the new id too: update_keypoint! left prev as it was
                j = i
            have.add(j)
            ids.append(j)
        assert len(set(ids)) == len(ids)
        order = np.argsort(np.array(ids, dtype=np.int64), kind="stable")
        return dict(Tcw=f["Tcw"], ids=np.array(ids, dtype=np.int64)[order], yx=f["yx"][order], is_3d=f["is_3d"][order], xyz=f["xyz"][order])

    def add(self, mask=None):
        self.sel = [True] * self.n if mask is None else [bool(v) for v in mask]
        took = {}
        for s in range(self.n):
            if not self.sel[s]:
                continue
            f, d = self.mapped(s, self.frames[s][self.nkf[s]]), self.descs[s][self.nkf[s]]
            nl.add_keyframe(self.m[s], self.D[s], self.nkf[s], f["Tcw"], f)
            nl.add_descriptors(self.m[s], self.D[s], d[0], d[1])
            self.lists[s] = dict(ids=f["ids"].copy(), yx=f["yx"].copy(), is_3d=f["is_3d"].copy(), xyz=f["xyz"].copy())
            took[s] = (f, d)
            self.nkf[s] += 1
        return took

    def merge(self, pairs, mutant=None):
        """the model's merge of per-stream pairs (an empty array: the stream is not acted on) -> the (S, 4) counts"""
        self.counts = np.zeros((self.n, 4), dtype=np.int32)
        for s in range(self.n):
            p = np.asarray(pairs[s], dtype=np.int64).reshape(-1, 2)
            if len(p) == 0:
                continue
            follow = self.mode == "follow"
            before = {a: self.m[s].entry(a) is not None for a in (int(v) for v in p[:, 0])}
            r = nm.merge(self.m[s], p, self.lists[s] if follow else None, with_list=follow, mutant=mutant, log=self.log[s])
            if follow and self.lists[s] is not None:
                self.lists[s] = r["list"]
            for a, b in ((int(a), int(b)) for a, b in p):
                if before[a] and self.m[s].entry(a) is None:     # applied: prev has left the table
                    self.ren[s][a] = b
            self.counts[s] = (r["applied"], r["skipped"], r["renamed"], r["status"])
        return self.counts

    def ba(self):
        """ModelRun.ba with the live lists following (mode "follow")"""
        out = {}
        for s in range(self.n):
            if not self.sel[s]:
                continue
            win = npk.gather(self.m[s])
            if win is None:
                continue
            theta, outl = scr.refined(self.seeds[s], win), scr.outlier_pattern(self.seeds[s], win)
            lst = npk.update(self.m[s], win, theta, outl, self.lists[s] if self.mode == "follow" else None)
            if lst is not None:
                self.lists[s] = lst
            out[s] = (win, theta, outl)
        return out

    def hand(self):
        """the hand-picked pairs of this key-frame, per stream (of the selected streams)"""
        out, kinds = [], []
        for s in range(self.n):
            p, k = hand_pairs(self.m[s]) if self.sel[s] else ([], [])
            out.append(np.array(p, dtype=np.int64).reshape(-1, 2)); kinds.append(k)
        return out, kinds


def run_sequence(run, on_step=None, mutant=None):
    """The sequence both test files run: every key-frame add -> match -> merge of the match's pairs; behind key-frame HAND_AT the hand-picked pairs; a
    local-BA update behind key-frames 3 and 4 (ls.BA_AT).  on_step(kind, k, data) is called after every step ("add", "match", "merge", "hand", "ba")."""
    for k in range(ls.N_KF):
        took = run.add(ls.LAST_MASK if k == ls.N_KF - 1 else None)
        on_step and on_step("add", k, took)
        res = run.match()
        on_step and on_step("match", k, res)
        pairs = [r["pairs"] if r["status"] == 0 else np.zeros((0, 2), dtype=np.int64) for r in res]
        run.merge(pairs, mutant=mutant)
        on_step and on_step("merge", k, pairs)
        if k == HAND_AT:
            hp, kinds = run.hand()
            run.merge(hp, mutant=mutant)
            on_step and on_step("hand", k, (hp, kinds))
        if k in ls.BA_AT:
            sol = run.ba()
            on_step and on_step("ba", k, sol)


# ---- the hand-built sequence at cap = 300 ------------------------------------------------------------------------------------------------------------------
HCAP, HR, HMCAP, HKF = 300, 4, 1024, 5
FLAT = (5, 421)                          # the 2-D points
# (prev, new): what the pair is there for.  Key-frame 4 is the newest (slot 0, which key-frame 0 held: id 50's observer slot has been reused).
HAND_PAIRS = [(400 + j, 100 + j) for j in range(20)] + [     # twenty renames per slab, from behind record 256 to before it: across the chunk edge
    (420, 3),                            # to the front of its slabs (3 is below every id they hold)
    (50, 500),                           # to the back of key-frames 2 and 3; key-frame 1 holds both: the has_new skip, an orphan stays
    (421, 4),                            # a 2-D prev
    (422, 5),                            # a new point that is not 3-D: skipped
    (423, 2000),                         # an id the map never held: skipped
    (424, 6)]                            # an id whose entry a larger id (1030) has taken: skipped
HAND_DEAD = [(400, 7), (60, 401)]        # behind the merge: a dead prev, a dead new -- both skipped


def hand_ids(k):
    ids = set(range(10 * k, 280 + 10 * k))
    if k >= 2:
        ids = (ids - set(range(100, 120))) | set(range(400, 420))
    if k == 1:
        ids.add(500)
    if k >= 3:
        ids |= set(range(420, 425))
    if k == 4:
        ids.add(1030)
    return np.array(sorted(ids), dtype=np.int64)


def hand_scene(seed=31):
    """-> frames [dict(Tcw, ids, yx, is_3d, xyz)] of key-frames 0 .. 4 of one stream; every number a function of (seed, id, key-frame)"""
    out = []
    for k in range(HKF):
        ids = hand_ids(k)
        assert len(ids) <= HCAP
        yx = np.array([[10.0 + 400.0 * scr._u(seed, 81, i, k), 10.0 + 600.0 * scr._u(seed, 82, i, k)] for i in ids])
        xyz = np.array([scr.world_point(seed, i) + 0.01 * scr._u(seed, 83, i, k) for i in ids])
        out.append(dict(Tcw=scr.pose(seed, k), ids=ids, yx=yx, is_3d=np.array([int(i) not in FLAT for i in ids], dtype=bool), xyz=xyz))
    return out


def hand_streams():
    """the S = 3 streams of the hand-built case: stream 0 has no pairs, streams 1 and 2 the pairs above (different numbers, the same ids)"""
    return [hand_scene(31 + s) for s in range(S)]
