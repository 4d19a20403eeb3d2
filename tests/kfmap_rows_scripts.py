"""Scripted sequences for the descriptor rows of the key-frame map (test helper): the scenes of tests/kfmap_lmm_scripts.py (S = 3, cap 64, R = 4,
mcap = 128, eight key-frames; the same lists, pixels and positions) with a descriptor script of its own, driven through tests/kfmap_merge_scripts.py's
sequence add -> add_descriptors -> match -> merge with the row model (tests/np_kfmap_rows.py) beside every map.

Descriptors: every new point draws a random 256-bit row; a COPY (the new points kfmap_lmm_scripts makes copies of an older point, twins included --
the choice of copies and targets is replayed from the frames with the same hashes) takes the NEWEST row of its target's chain with exactly 60 bits
flipped: generation g of a chain flips bits [60 g, 60 g + 60) mod 256, so one generation apart the distance is 60 <= 89.6 = 256 * 0.35 and two apart
it is 120 > 89.6.  A chain is an original and the copies made of it: a point that is lost, seen again under a new id (merged), and seen again later
has drifted two generations from its first row and pairs through the row the merge handed over, or not at all.

drift_stream(): the hand-built stream of that case alone.  Point A is born at key-frame 0 and seen by key-frame 1; re-detection B (generation 1)
arrives at key-frame 2 and is merged into A; re-detection C (generation 2) arrives at key-frame 4, whose slot (R = 4) is key-frame 0's: A's own row
has gone with that observation and C pairs through B's row alone."""
import numpy as np

import kfmap_lmm_scripts as ls
import kfmap_merge_scripts as ms
import kfmap_scripts as scr
import np_kfmap as npk
import np_kfmap_filter as npf
import np_kfmap_rows as nr

S = ls.S
FLIP = 60


def generation(row, g):
    """the row of the next generation g >= 1 of a chain: bits [60 g, 60 g + 60) mod 256 of `row` flipped"""
    out = [int(v) for v in row]
    for t in range(FLIP):
        b = (FLIP * g + t) % 256
        out[b >> 6] ^= 1 << (b & 63)
    return np.array(out, dtype=np.uint64)


def hamming(a, b):
    return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))


def rows_descs(seed, frames, p_copy=0.45, window=3):
    """-> (descs, copies): descs[k] = (first new id, (n_new, 4) rows) as kfmap_lmm_scripts.make_scene's, with this module's rows; copies: id ->
    (target, root of the chain, generation).  The copies and their targets are make_scene's, replayed from its frames."""
    known, last_seen, seen = {}, {}, set()
    rows, root, newest, copies, descs = {}, {}, {}, {}, []
    for k, f in enumerate(frames):
        ids = [int(i) for i in f["ids"]]
        new = [i for i in ids if i not in seen]
        targets = []
        for t in sorted(known):
            if t in ids or k - last_seen[t] > window:
                continue
            p = ls.project(f["Tcw"], known[t])
            if p is not None and 2.0 <= p[0] <= ls.H - 1.0 and 2.0 <= p[1] <= ls.W - 1.0:
                targets.append(t)
        for i in new:
            rows[i], root[i] = ls.random_row(seed, i), i
            if k > 0 and targets and scr._u(seed, 64, i) < p_copy:
                t = targets[int(scr._u(seed, 65, i) * len(targets))]
                r = root[t]
                g = newest[r][1] + 1
                rows[i], root[i] = generation(newest[r][0], g), r
                newest[r] = (rows[i], g)
                copies[i] = (t, r, g)
            else:
                newest[i] = (rows[i], 0)
        for j, i in enumerate(ids):
            seen.add(i); last_seen[i] = k
            if f["is_3d"][j]:
                known[i] = f["xyz"][j].copy()
        descs.append((new[0] if new else (max(seen) + 1 if seen else 0), np.array([rows[i] for i in new], dtype=np.uint64).reshape(-1, 4)))
    return descs, copies


def scenes():
    frames, _ = ls.scenes()
    made = [rows_descs(seed, fr) for seed, fr in zip(ls.SEEDS, frames)]
    return frames, [m[0] for m in made], [m[1] for m in made]


class RowsRun(ms.MergeRun):
    """MergeRun on this module's descriptor script.  max_rows = D: the row model beside every map (np_kfmap_rows); max_rows = None: the one-row
    models as they are (np_kfmap_local_map / np_kfmap_merge), on the same script.  frames / descs: other scenes than scenes()."""

    def __init__(self, mode, max_rows, frames=None, descs=None, mutant=None, **kw):
        super().__init__(mode, **kw)
        if frames is None:
            frames, descs, self.copies = scenes()
        self.frames, self.descs, self.n = frames, descs, len(frames)
        self.max_rows, self.mutant = max_rows, mutant
        if max_rows is not None:
            self.D = [nr.new_descriptors(m, max_rows) for m in self.m]

    def add(self, mask=None):
        if self.max_rows is None:
            return super().add(mask)
        self.sel = [True] * self.n if mask is None else [bool(v) for v in mask]
        took = {}
        for s in range(self.n):
            if not self.sel[s]:
                continue
            f, d = self.mapped(s, self.frames[s][self.nkf[s]]), self.descs[s][self.nkf[s]]
            nr.add_keyframe(self.m[s], self.D[s], self.nkf[s], f["Tcw"], f, mutant=self.mutant)
            nr.add_descriptors(self.m[s], self.D[s], d[0], d[1])
            self.lists[s] = dict(ids=f["ids"].copy(), yx=f["yx"].copy(), is_3d=f["is_3d"].copy(), xyz=f["xyz"].copy())
            took[s] = (f, d)
            self.nkf[s] += 1
        return took

    def match(self, max_local=None):
        if self.max_rows is None:
            return super().match(max_local=max_local)
        idle = nr.local_map_match(npk.Map(1, 2, 1), None, ls.CAM10, ls.CELL, ls.PARAMS)
        return [nr.local_map_match(self.m[s], self.D[s], ls.CAM10, ls.CELL, ls.PARAMS, max_local=max_local) if self.sel[s] else idle for s in range(self.n)]

    def merge(self, pairs, mutant=None):
        if self.max_rows is None:
            return super().merge(pairs)
        self.counts = np.zeros((self.n, 4), dtype=np.int32)
        follow = self.mode == "follow"
        for s in range(self.n):
            p = np.asarray(pairs[s], dtype=np.int64).reshape(-1, 2)
            if len(p) == 0:
                continue
            before = {a: self.m[s].entry(a) is not None for a in (int(v) for v in p[:, 0])}
            r = nr.merge(self.m[s], self.D[s], p, self.lists[s] if follow else None, with_list=follow, mutant=self.mutant, log=self.log[s])
            if follow and self.lists[s] is not None:
                self.lists[s] = r["list"]
            for a, b in ((int(a), int(b)) for a, b in p):
                if before[a] and self.m[s].entry(a) is None:
                    self.ren[s][a] = b
            self.counts[s] = (r["applied"], r["skipped"], r["renamed"], r["status"])
        return self.counts

    def ba(self):
        if self.max_rows is None:
            return super().ba()
        out = {}
        for s in range(self.n):
            if not self.sel[s]:
                continue
            win = nr.gather(self.m[s], self.D[s], mutant=self.mutant)
            if win is None:
                continue
            theta, outl = scr.refined(self.seeds[s], win), scr.outlier_pattern(self.seeds[s], win)
            lst = nr.update(self.m[s], self.D[s], win, theta, outl, self.lists[s] if self.mode == "follow" else None, mutant=self.mutant)
            if lst is not None:
                self.lists[s] = lst
            out[s] = (win, theta, outl)
        return out

    def filter(self, ratio, minc, first_kfid=0):
        """the model's map_filtering! on the selected streams -> per stream the log of np_kfmap_filter.filter_map"""
        logs = []
        for s in range(self.n):
            if not self.sel[s]:
                logs.append([])
            elif self.max_rows is None:
                logs.append(npf.filter_map(self.m[s], ratio, int(minc[s]), first_kfid=first_kfid))
            else:
                logs.append(nr.filter_map(self.m[s], self.D[s], ratio, int(minc[s]), first_kfid=first_kfid, mutant=self.mutant))
        return logs

    def rows(self, s):
        return nr.descriptor_rows(self.m[s], self.D[s])


def run_sequence(run, on_step=None):
    """kfmap_merge_scripts.run_sequence (add -> match -> merge at every key-frame, the hand-picked merge, the updates behind key-frames 3 and 4), then
    a filter that removes every covisible key-frame it may (min_cov_score far above every count) and once more match and merge on what is left.
    -> every pair the matches found, as (key-frame, stream, keypoint id, local-map id)"""
    found = []

    def step(kind, k, data):
        if kind == "match":
            found.extend((k, s, int(a), int(b)) for s, r in enumerate(data) if r["status"] == 0 for a, b in r["pairs"])
        on_step and on_step(kind, k, data)
    ms.run_sequence(run, step)
    logs = run.filter(0.5, [1000] * run.n)
    step("filter", ls.N_KF, logs)
    res = run.match()
    step("match", ls.N_KF, res)
    run.merge([r["pairs"] if r["status"] == 0 else np.zeros((0, 2), dtype=np.int64) for r in res])
    step("merge", ls.N_KF, None)
    return found


def orphaned_by_filter(m, logs_removed):
    """the live points of map m (before the filter) whose valid observers are all among the key-frames `logs_removed`, two or more of them"""
    gone = set(int(k) for k in logs_removed)
    out = []
    for e in range(m.mcap):
        if m.ptag[e] >= 0 and not m.flags[e] & npk.F_DEAD:
            obs = set(m.observers(e))
            if len(obs) >= 2 and obs <= gone:
                out.append(int(m.ptag[e]))
    return out


# ---- the hand-built drift stream ---------------------------------------------------------------------------------------------------------------------------
DRIFT_A, DRIFT_B, DRIFT_C = 5, 40, 80
DRIFT_KF = 5


def drift_stream(seed=41):
    """-> (frames, descs) of key-frames 0 .. 4 of one stream at kfmap_lmm_scripts' camera: ten background points per key-frame (ids 10 k .. 10 k + 9,
    seen by key-frames k and k + 1, so that consecutive key-frames are covisible), A = 5 in key-frames 0 and 1, B = 40 in 2 and 3, C = 80 in 4; B
    and C are A seen again (its position, a pixel at its projection) and carry generations 1 and 2 of A's row"""
    Xa = np.array([0.05, -0.04, 2.0])
    frames, descs, row_a = [], [], ls.random_row(seed, DRIFT_A)
    row_b = generation(row_a, 1)
    row_c = generation(row_b, 2)
    special = {DRIFT_A: row_a, DRIFT_B: row_b, DRIFT_C: row_c}
    seen = set()
    for k in range(DRIFT_KF):
        T = np.eye(4); T[0, 3] = 0.01 * k
        ids = set(range(10 * k, 10 * k + 10)) | (set(range(10 * (k - 1), 10 * k)) if k else set())
        ids -= {DRIFT_A, DRIFT_B, DRIFT_C}
        ids |= {DRIFT_A} if k in (0, 1) else {DRIFT_B} if k in (2, 3) else {DRIFT_C}
        ids = sorted(ids)
        pa = ls.project(T, Xa)
        yx, xyz = [], []
        for i in ids:
            if i in special:
                yx.append(pa + 0.3 * np.array([scr._u(seed, 91, i, k) - 0.5, scr._u(seed, 92, i, k) - 0.5])); xyz.append(Xa.copy())
            else:
                yx.append(np.array([1.5 + (ls.H - 2.0) * scr._u(seed, 93, i, k), 1.5 + (ls.W - 2.0) * scr._u(seed, 94, i, k)]))
                xyz.append(np.array([4.0 * scr._u(seed, 95, i) - 2.0, 4.0 * scr._u(seed, 96, i) - 2.0, 30.0 + 5.0 * scr._u(seed, 97, i)]))
        new = [i for i in ids if i not in seen]
        seen |= set(ids)
        frames.append(dict(Tcw=T, ids=np.array(ids, dtype=np.int64), yx=np.array(yx).reshape(-1, 2), is_3d=np.ones(len(ids), dtype=bool), xyz=np.array(xyz).reshape(-1, 3)))
        first = new[0]
        rows = np.array([special.get(i, ls.random_row(seed, i)) for i in range(first, new[-1] + 1)], dtype=np.uint64).reshape(-1, 4)
        descs.append((first, rows))
    return frames, descs
