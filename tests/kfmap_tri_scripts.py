"""Scripted sequences for temporal triangulation on the key-frame map (test helper): tests/test_kfmap_tri_host.py runs them on the model
(tests/np_kfmap_tri.py over tests/np_kfmap.py), tests/test_gpu_kfmap_tri.py on the device beside the model.

Scenes: mono lists -- every keypoint is born 2-D, so 2-D points survive to a second key-frame -- of world points seen through a pinhole camera that
moves sideways and forward with a little yaw (the poses of test_temporal_triangulation_on_the_set_equals_the_host_seam).  Pixel noise is 0.2 px
(uniform); about 15 % of a key-frame's observations are displaced by 25-60 px per axis, so that gates fail with a parallax above 20, and a further
10 % by 5-12 px in y, across the epipolar lines of the sideways motion, so that gates also fail BELOW the parallax bar (far points: accepted as
they are).  Every number is a function of (seed, stream, id, key-frame).

TriRun holds S models, their live lists and (optionally) their descriptor rows, and offers the steps the sequences are made of: add, tri,
remove_keyframe, gather, update, merge.  A sequence is a function of a run; it calls run.step(name) after every step, where the GPU test compares the
device with the model.  SEQUENCES maps a name to (constructor arguments, function).

scene_ok(run) is the scenes' guard: every gate quantity of every candidate a sequence met stays 1e-6 (px or m) away from its threshold and the
rotated bearing's z component stays at least 0.1 away from zero; make(name) regenerates with the next seed while it does not hold, three seeds at most.
  why 1e-6: the device and numpy differ only by f64 rounding of sin / cos and 4 x 4 products on pixel magnitudes of about 1e3, about 1e-12 px, so
  1e-6 excludes no honest case and hides no wrong one."""
import numpy as np

import kfmap_scripts as scr
import np_kfmap as npk
import np_kfmap_filter as npf
import np_kfmap_local_map as nl
import np_kfmap_merge as nm
import np_kfmap_rows as nr
import np_kfmap_tri as nt

CAM = (718.856, 718.856, 607.1928, 185.2157)
CAP, R, MCAP = 64, 4, 256
MARGIN, BZ_GUARD, MAX_SEEDS = 1e-6, 0.1, 3
MINC = 5                                 # min_cov_score of the sequences that gather
MAX_ERROR, MIN_DEPTH, MIN_PARALLAX = 3.0, 0.1, 20.0


def pose(k, s):
    """Tcw of key-frame k of stream s: sideways and forward, a little yaw"""
    th = 0.01 * k
    T = np.eye(4)
    T[:3, :3] = [[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]]
    T[:3, 3] = [-0.6 * k - 0.1 * s, 0.02 * k, -0.3 * k]
    return T


def world_point(seed, i):
    return np.array([-15.0 + 30.0 * scr._u(seed, 1, i), -4.0 + 8.0 * scr._u(seed, 2, i), 6.0 + 54.0 * scr._u(seed, 3, i)])


def pixel(seed, s, i, k):
    """the observation of point i in key-frame k: projection + 0.2 px of noise; about 15 % displaced by 25-60 px per axis"""
    T = pose(k, s)
    Xc = T[:3, :3] @ world_point(seed, i) + T[:3, 3]
    yx = np.array([CAM[1] * Xc[1] / Xc[2] + CAM[3], CAM[0] * Xc[0] / Xc[2] + CAM[2]])
    yx += 0.4 * (np.array([scr._u(seed, 21, i, k), scr._u(seed, 22, i, k)]) - 0.5)
    if scr._u(seed, 23, i, k) < 0.15:
        sgn = np.where(np.array([scr._u(seed, 24, i, k), scr._u(seed, 25, i, k)]) < 0.5, -1.0, 1.0)
        yx += sgn * (25.0 + 35.0 * np.array([scr._u(seed, 26, i, k), scr._u(seed, 27, i, k)]))
    elif scr._u(seed, 28, i, k) < 0.10:                          # a further 10 %: 5-12 px across the epipolar lines -- a gate fails, on far points below the parallax bar
        yx[0] += (1.0 if scr._u(seed, 29, i, k) < 0.5 else -1.0) * (5.0 + 7.0 * scr._u(seed, 30, i, k))
    return yx


def tracks(seed, sizes, p_drop=0.2):
    """-> per key-frame the ascending ids of the scripted list: tracks drop out by hash, newborn ids (larger than every earlier one) fill up to sizes[k]"""
    alive, next_id, out = [], 0, []
    for k, n in enumerate(sizes):
        keep = [i for i in alive if scr._u(seed, 11, i, k) >= p_drop]
        while len(keep) > n:
            keep.pop(int(scr._u(seed, 12, len(keep), k) * len(keep)))
        born = next_id
        while len(keep) < n:
            keep.append(next_id); next_id += 1
        alive = keep
        out.append((np.array(alive, dtype=np.int64), born))
    return out


class TriRun:
    """S models with their live lists.  lists[s]: what KeypointSet.download must return for stream s (None before its first key-frame)."""

    def __init__(self, sizes, seed=0, cap=CAP, R=R, mcap=MCAP, rows=0, minc=MINC, with_list=True, p_drop=0.2):
        self.S, self.cap, self.R, self.mcap, self.rows, self.minc, self.with_list = len(sizes), cap, R, mcap, rows, minc, with_list
        self.seed = seed
        self.seeds = [1000 * seed + 17 * s + 3 for s in range(self.S)]
        self.tracks = [tracks(self.seeds[s], sizes[s], p_drop) for s in range(self.S)]
        self.m = [npk.Map(cap, R, mcap, CAM, None, minc) for _ in range(self.S)]
        self.D = [nr.new_descriptors(m, rows) for m in self.m] if rows else None
        self.lists = [None] * self.S
        self.nkf = [0] * self.S
        self.sel = [True] * self.S
        self.met = []                    # every candidate dict the tri steps returned
        self.last = None                 # the last tri step's per-stream results (None: not acted on)
        self.on_step = None

    def step(self, name):
        if self.on_step:
            self.on_step(name)

    # ---- steps ----
    def next_list(self, s):
        """the list of stream s's next key-frame: the scripted ids the live list still holds or that are born now, in id order; is_3d and xyz as
        the live list has them"""
        k = self.nkf[s]
        ids, born = self.tracks[s][k]
        old = self.lists[s]
        have = {} if old is None else {int(i): j for j, i in enumerate(old["ids"])}
        ids = np.array([i for i in ids if int(i) >= born or int(i) in have], dtype=np.int64)
        yx = np.array([pixel(self.seeds[s], s, int(i), k) for i in ids]).reshape(-1, 2)
        is3 = np.array([bool(old["is_3d"][have[int(i)]]) if int(i) in have else False for i in ids], dtype=bool)
        xyz = np.array([old["xyz"][have[int(i)]] if int(i) in have else np.zeros(3) for i in ids]).reshape(-1, 3)
        return dict(Tcw=pose(k, s), ids=ids, yx=yx, is_3d=is3, xyz=xyz)

    def add(self, mask=None):
        """the next key-frame of every selected stream -> {s: the list}"""
        self.sel = [True] * self.S if mask is None else [bool(v) for v in mask]
        took = {}
        for s in range(self.S):
            if not self.sel[s]:
                continue
            f = self.next_list(s)
            lst = dict(ids=f["ids"], yx=f["yx"], is_3d=f["is_3d"], xyz=f["xyz"])
            if self.rows:
                nr.add_keyframe(self.m[s], self.D[s], self.nkf[s], f["Tcw"], lst)
                born = self.tracks[s][self.nkf[s]][1]
                new = [int(i) for i in f["ids"] if int(i) >= born]
                if new:                                          # the newborn ids are consecutive: one block of rows, as detect_describe hands them over
                    nr.add_descriptors(self.m[s], self.D[s], new[0], self.desc_rows(s, new))
            else:
                npk.add_keyframe(self.m[s], self.nkf[s], f["Tcw"], lst)
            self.lists[s] = {k: v.copy() for k, v in lst.items()}
            took[s] = f
            self.nkf[s] += 1
        return took

    def desc_rows(self, s, ids):
        return np.array([[int(scr._u(self.seeds[s], 61, i, w) * (1 << 53)) for w in range(4)] for i in ids], dtype=np.uint64).reshape(-1, 4)

    def tri(self, mutant=None, with_list=None):
        """the model's triangulation for the streams of the last add -> per stream the result dict (None: not acted on)"""
        with_list = self.with_list if with_list is None else with_list
        out = []
        for s in range(self.S):
            if not self.sel[s]:
                out.append(None)
                continue
            lst = self.lists[s] if with_list else None
            if self.rows:                                        # (the rows follow the observer bit the rejection clears: np_kfmap_rows.upkeep)
                r = nr.through(nt.triangulate_temporal)(self.m[s], self.D[s], CAM, lst, MAX_ERROR, MIN_DEPTH, MIN_PARALLAX)
            else:
                r = nt.triangulate_temporal(self.m[s], CAM, lst, MAX_ERROR, MIN_DEPTH, MIN_PARALLAX, mutant=mutant)
            if with_list and r["list"] is not None:
                self.lists[s] = r["list"]
            self.met += r["cand"]
            out.append(r)
        self.last = out
        return out

    def remove_keyframe(self, s, kfid):
        if self.rows:
            nr.remove_keyframe(self.m[s], self.D[s], kfid)
        else:
            npf.remove_keyframe(self.m[s], kfid)

    def gather(self):
        """-> {s: window} of the selected streams that have one"""
        out = {}
        for s in range(self.S):
            if self.sel[s]:
                w = nr.gather(self.m[s], self.D[s]) if self.rows else npk.gather(self.m[s])
                if w is not None:
                    out[s] = w
        return out

    def solution(self, s, win, outliers=None):
        """a stand-in for the solver: theta moved by a hash of its index (1e-3: the refined poses and points differ visibly), outliers by hash or as
        given: a set of (key-frame, keypoint)"""
        theta = scr.refined(self.seeds[s], win)
        if outliers is None:
            outl = scr.outlier_pattern(self.seeds[s], win)
        else:
            outl = np.array([(int(a), int(b)) in outliers for a, b in zip(win["obs_kf"], win["obs_kp"])], dtype=bool)
        return theta, outl

    def update(self, wins, sols):
        for s, win in wins.items():
            theta, outl = sols[s]
            a = (self.m[s], self.D[s]) if self.rows else (self.m[s],)
            lst = (nr.update if self.rows else npk.update)(*a, win, theta, outl, self.lists[s] if self.with_list else None)
            if lst is not None:
                self.lists[s] = lst

    def merge(self, pairs):
        """per-stream (prev, new) pairs (an empty array: not acted on) -> (S, 4) counts"""
        counts = np.zeros((self.S, 4), dtype=np.int32)
        for s in range(self.S):
            p = np.asarray(pairs[s], dtype=np.int64).reshape(-1, 2)
            if len(p) == 0:
                continue
            a = (self.m[s], self.D[s]) if self.rows else (self.m[s],)
            r = (nr.merge if self.rows else nm.merge)(*a, p, self.lists[s] if self.with_list else None, with_list=self.with_list)
            if self.with_list:
                self.lists[s] = r["list"]
            counts[s] = (r["applied"], r["skipped"], r["renamed"], r["status"])
        return counts


def codes(res):
    """{code: number of candidates} of one stream's tri result"""
    out = {}
    for c in res["cand"]:
        out[c["code"]] = out.get(c["code"], 0) + 1
    return out


# ---- the sequences: each a function of a run; run.step(name) after every step ---------------------------------------------------------------------------
def seq_plain(run):
    """1: KF0 then KF1; points detected at KF1 have one observer and are skipped"""
    run.add(); run.step("add0")
    run.tri(); run.step("tri0")                                  # every candidate's first observer is the key-frame itself
    run.add(); run.step("add1")
    run.tri(); run.step("tri1")


def seq_withheld(run):
    """2: triangulation withheld until KF2, then remove_keyframe(0) first: the observer is 1"""
    for k in range(3):
        run.add(); run.step("add%d" % k)
    for s in range(run.S):
        run.remove_keyframe(s, 0)
    run.step("remove0")
    run.tri(); run.step("tri2")


def seq_ring(run):
    """3: R = 4, key-frames 0-4 with triangulation withheld: slot 0 is reused and the observer is 1"""
    for k in range(5):
        run.add(); run.step("add%d" % k)
    run.tri(); run.step("tri4")


def seq_refined(run):
    """4: a gather and an update with perturbed theta before the call: the world points move with the refined pose"""
    run.add(); run.step("add0")
    run.add(); run.step("add1")
    run.tri(); run.step("tri1")                                  # 3-D points for the window
    run.add(); run.step("add2")
    wins = run.gather(); run.step("gather2")
    run.update(wins, {s: run.solution(s, w, outliers=set()) for s, w in wins.items()}); run.step("update2")
    run.tri(); run.step("tri2")


def seq_tombstones(run):
    """5, as far as the seams reach: a point rejected at key-frame 1 has a tombstone there and its bit cleared; seen again at key-frames 2 and 3 its
    observers are 0, 2, 3 and the pair is (0, 3).  An update that tombstones every observation its window holds in key-frame 1 (3-D points: a window
    holds no 2-D point) runs before the call and must not disturb it.  The two states the seams cannot produce for a 2-D point -- a tombstone in the
    first observer's slab under a set bit, an observer bit cleared by update -- are set by hand on the model in tests/test_kfmap_tri_host.py."""
    run.add(); run.step("add0")
    run.add(); run.step("add1")
    run.tri(); run.step("tri1")
    run.add(); run.step("add2")
    run.add(); run.step("add3")                                  # (triangulation withheld at key-frame 2)
    wins = run.gather(); run.step("gather3")
    sols = {}
    for s, w in wins.items():
        theta, outl = run.solution(s, w)
        sols[s] = (w["theta"].copy(), outl | (np.asarray(w["obs_kf"]) == 1))
    run.update(wins, sols); run.step("update3")
    run.tri(); run.step("tri3")


def seq_table(run):
    """6: mcap = 16, so newer ids take entries: orphans and dead points are skipped"""
    for k in range(3):
        run.add(); run.step("add%d" % k)
        run.tri(); run.step("tri%d" % k)
    wins = run.gather(); run.step("gather2")
    run.update(wins, {s: run.solution(s, w) for s, w in wins.items()}); run.step("update2")         # removes points: dead entries
    run.add(); run.step("add3")
    run.tri(); run.step("tri3")


def seq_selection(run):
    """7: the middle stream of S = 3 is unselected at the last add_keyframe"""
    run.add(); run.step("add0")
    run.add(); run.step("add1")
    run.add([1, 0, 1]); run.step("add2")
    run.tri(); run.step("tri2")


def seq_wide(run):
    """8: cap = 300 with 257-300 observations in the newest slab: a stream spans two workgroups"""
    run.add(); run.step("add0")
    run.add(); run.step("add1")
    run.tri(); run.step("tri1")


def seq_rows(run):
    """9: the row store on (D = 2): a removed observation drops the row keyed k and dhas stays"""
    for k in range(3):
        run.add(); run.step("add%d" % k)
        run.tri(); run.step("tri%d" % k)


def seq_pending(run):
    """10: a call between gather and update: the pending window is applied unchanged"""
    run.add(); run.step("add0")
    run.add(); run.step("add1")
    run.tri(); run.step("tri1")
    run.add(); run.step("add2")
    wins = run.gather(); run.step("gather2")
    sols = {s: run.solution(s, w) for s, w in wins.items()}
    run.tri(); run.step("tri2")
    run.update(wins, sols); run.step("update2")


def merge_pairs(run):
    """per stream: a keypoint born at the newest key-frame (prev) onto a 3-D point the newest key-frame does not observe (new, a smaller id): the
    list's slot takes the smaller id and moves forward, so list index != slab index behind it"""
    out = []
    for s in range(run.S):
        m = run.m[s]
        r0 = m.cur % m.R
        newest = set(int(i) for i in m.ids[r0, :int(m.n[r0])])
        born = run.tracks[s][run.nkf[s] - 1][1]
        prev = [i for i in sorted(newest) if i >= born and m.entry(i) is not None]
        new = [int(m.ptag[e]) for e in range(m.mcap) if m.ptag[e] >= 0 and not m.flags[e] & npk.F_DEAD and m.flags[e] & npk.F_3D and int(m.ptag[e]) not in newest]
        n = min(len(prev), len(new), 3)
        out.append(np.array(list(zip(prev[-n:], sorted(new)[:n])), dtype=np.int64).reshape(-1, 2))
    return out


def seq_merged(run):
    """11: with and without a list, after a BA update has compacted the list and a merge has re-ordered it: list index != slab index"""
    run.add(); run.step("add0")
    run.add(); run.step("add1")
    run.tri(); run.step("tri1")
    run.add(); run.step("add2")
    wins = run.gather(); run.step("gather2")
    run.update(wins, {s: run.solution(s, w) for s, w in wins.items()}); run.step("update2")
    run.pairs = merge_pairs(run)
    run.merge(run.pairs); run.step("merge2")
    run.tri(); run.step("tri2")


S3 = lambda *sizes: tuple(tuple(z) for z in sizes)
SEQUENCES = {
    "plain": (dict(sizes=S3((50, 60), (40, 64), (30, 45))), seq_plain),
    "withheld": (dict(sizes=S3((50, 55, 60), (40, 50, 64))), seq_withheld),
    "ring": (dict(sizes=S3((50, 52, 54, 56, 60), (40, 45, 50, 55, 64))), seq_ring),
    "refined": (dict(sizes=S3((50, 55, 60), (40, 50, 64))), seq_refined),
    "tombstones": (dict(sizes=S3((50, 52, 54, 56), (40, 45, 50, 55))), seq_tombstones),
    "table": (dict(sizes=S3((14, 15, 16, 16), (12, 14, 15, 16)), mcap=16), seq_table),
    "selection": (dict(sizes=S3((50, 55, 60), (40, 50, 64), (30, 40, 45))), seq_selection),
    "wide": (dict(sizes=S3((300, 300), (290, 280)), cap=300, mcap=1024, p_drop=0.05), seq_wide),       # few drops: tracked points behind observation 256
    "rows": (dict(sizes=S3((50, 55, 60), (40, 50, 64)), rows=2), seq_rows),
    "no_rows": (dict(sizes=S3((50, 55, 60), (40, 50, 64))), seq_rows),
    "pending": (dict(sizes=S3((50, 55, 60), (40, 50, 64))), seq_pending),
    "merged": (dict(sizes=S3((50, 55, 60), (40, 50, 64))), seq_merged),
    "merged_no_list": (dict(sizes=S3((50, 55, 60), (40, 50, 64)), with_list=False), seq_merged),
}
UNBOUNDED = ("plain", "refined", "tombstones", "pending")      # nothing is forgotten: no ring reuse, no table wrap, no removed key-frame, no merge


def scene_ok(run):
    return all(c["margin"] >= MARGIN and abs(c["bz"]) >= BZ_GUARD for c in run.met)


def make(name, cls=TriRun, **kw):
    """a fresh run of sequence `name` whose scene passes the guard (found on the model alone) -> (run, fn); the run has not been driven yet"""
    args, fn = SEQUENCES[name]
    for seed in range(MAX_SEEDS):
        probe = TriRun(seed=seed, **args)
        fn(probe)
        if scene_ok(probe):
            return cls(seed=seed, **args, **kw), fn
    raise AssertionError("sequence %s: no scene within %d seeds keeps its gates %g away from their thresholds" % (name, MAX_SEEDS, MARGIN))
