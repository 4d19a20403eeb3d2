"""Scripted scenes for the key-frame map behind a lens (test helper): the scenes of tests/kfmap_lmm_scripts.py with every list pixel p replaced by the
RAW pixel a camera with lens distortion would report for it, pdn_to_pixel(cam, dist, (p_y - cy) / fy, (p_x - cx) / fx) (csrc/geom_device.hpp), and the
model of a map that keeps that raw pixel beside the undistorted one (slam_kfmap_enable_pixels).  Lists, ids, positions, descriptors and the sequence
(N_KF = 8, LAST_MASK, BA_AT) are kfmap_lmm_scripts'.

The model keeps TWO pixel arrays per slab, index for index: m.upx = undistort(raw) -- np_kfmap's own, read by the gather, hence by the local BA -- and
m.views["raw"], the list's pixel as it was, read by the match (find_best_match and the frame grid work on kp.pixel, mapper.jl:405-442,
frame.jl:576-599).  The models of the match (np_kfmap_local_map, np_kfmap_local_map_history, np_kfmap_rows) read m.upx: matching(m, view) hands them
the map with the chosen array in that place for the length of a call.  A merge moves a view as np_kfmap_merge moves upx: the same model run on a copy
of the map that carries the view as its pixels.  m.views["pinhole"] holds the scene's pixel before the lens, for the mutants:

  mutant A   raw pixels, a pinhole camera in the match        (the lens forgotten in the projection)
  mutant B   pinhole pixels, the lens camera in the match     (the lens forgotten in the pixels)
  mutant U   the undistorted pixels, the lens camera          (a stager that reads kupx where it should read kpx)

With dist all zero no pixel changes and the model equals the one without the store, bit for bit."""
import contextlib
import copy

import numpy as np

import kfmap_lmm_scripts as ls
import kfmap_merge_scripts as ms
import kfmap_rows_scripts as rs
import np_kfmap as npk
import np_kfmap_local_map as nl
import np_kfmap_local_map_history as nh
import np_kfmap_merge as nm
import np_kfmap_rows as nr

DIST = (-0.28, 0.07, 2e-4, 2e-5)
ZERO = (0.0, 0.0, 0.0, 0.0)
CAM4 = ls.CAM10[:4]
KINDS = ("plain", "history", "rows")
EMPTY = np.zeros((0, 2), dtype=np.int64)


def cam10(dist):
    return CAM4 + tuple(float(v) for v in dist) + ls.CAM10[8:]


def lens_pixel(dist, yx):
    """the raw pixel of pinhole pixel yx; without a lens the pixel itself"""
    yx = np.asarray(yx, dtype=np.float64).reshape(-1, 2)
    return npk.undistort(CAM4, dist, yx) if np.any(dist) else yx.copy()


def lens_frames(frames, dist):
    """the scenes' frames with raw pixels; "pinhole": the pixel before the lens"""
    return [[dict(f, yx=lens_pixel(dist, f["yx"]), pinhole=f["yx"].copy()) for f in fr] for fr in frames]


@contextlib.contextmanager
def matching(maps, view):
    """the maps with views[view] where the match's models read their pixels (view "upx": the maps as they are)"""
    kept = [m.upx for m in maps]
    try:
        if view != "upx":
            for m in maps:
                m.upx = m.views[view]
        yield
    finally:
        for m, u in zip(maps, kept):
            m.upx = u


class LensRun(ms.MergeRun):
    """MergeRun on the lens scenes with the raw-pixel views beside every map.  kind: "plain" (np_kfmap_local_map), "history" (the local-map history,
    merges without a list) or "rows" (np_kfmap_rows with max_rows).  match(view, lens): which pixels the match reads and whether its camera has the lens."""

    def __init__(self, dist=DIST, mode="stale", kind="plain", max_rows=2):
        assert kind in KINDS
        frames, descs = rs.scenes()[:2] if kind == "rows" else ls.scenes()
        ls.ModelRun.__init__(self, lens_frames(frames, dist), descs)
        self.mode, self.kind, self.dist, self.cam = ("stale" if kind == "history" else mode), kind, tuple(dist), cam10(dist)
        self.lists = [None] * self.n
        self.ren = [dict() for _ in range(self.n)]
        self.log = [dict() for _ in range(self.n)]
        self.counts = np.zeros((self.n, 4), dtype=np.int32)
        self.m = [npk.Map(ls.CAP, ls.R, ls.MCAP, CAM4, dist, m.min_cov_score) for m in self.m]
        for m in self.m:
            m.views = {"raw": np.zeros((m.R, m.cap, 2)), "pinhole": np.zeros((m.R, m.cap, 2))}
        self.D = [nr.new_descriptors(m, max_rows) if kind == "rows" else nl.new_descriptors(m) for m in self.m]
        self.H = [nh.History(ls.R) for _ in self.m]

    def add(self, mask=None):
        self.sel = [True] * self.n if mask is None else [bool(v) for v in mask]
        took = {}
        for s in range(self.n):
            if not self.sel[s]:
                continue
            m, k = self.m[s], self.nkf[s]
            src = self.frames[s][k]
            f, d = self.mapped(s, src), self.descs[s][k]
            if self.kind == "rows":
                nr.add_keyframe(m, self.D[s], k, f["Tcw"], f)
                nr.add_descriptors(m, self.D[s], d[0], d[1])
            else:
                nl.add_keyframe(m, self.D[s], k, f["Tcw"], f)
                nl.add_descriptors(m, self.D[s], d[0], d[1])
            n = len(f["ids"])
            m.views["raw"][k % m.R, :n] = f["yx"]                # the list's pixel as it is, beside upx = undistort of it
            if f is src:                                         # (a list the renames re-ordered has no scene pixel: the mutants run without merges)
                m.views["pinhole"][k % m.R, :n] = src["pinhole"]
            self.lists[s] = dict(ids=f["ids"].copy(), yx=f["yx"].copy(), is_3d=f["is_3d"].copy(), xyz=f["xyz"].copy())
            took[s] = (f, d)
            self.nkf[s] += 1
        return took

    def match(self, max_local=None, view="raw", lens=True):
        cam = self.cam if lens else ls.CAM10
        with matching(self.m, view):
            if self.kind == "history":
                idle = dict(nh._none(), C=[], size=0, chain=[], branch=None)
                fn = lambda s: nh.local_map_match(self.m[s], self.D[s], self.H[s], cam, ls.CELL, ls.PARAMS, max_local=max_local)      # noqa: E731
            elif self.kind == "rows":
                idle = nr.local_map_match(npk.Map(1, 2, 1), None, cam, ls.CELL, ls.PARAMS)
                fn = lambda s: nr.local_map_match(self.m[s], self.D[s], cam, ls.CELL, ls.PARAMS, max_local=max_local)                 # noqa: E731
            else:
                idle = nl.local_map_match(npk.Map(1, 2, 1), None, cam, ls.CELL, ls.PARAMS)
                fn = lambda s: nl.local_map_match(self.m[s], self.D[s], cam, ls.CELL, ls.PARAMS, max_local=max_local)                 # noqa: E731
            return [fn(s) if self.sel[s] else idle for s in range(self.n)]

    def merge(self, pairs, mutant=None):
        """the model's merge; every view follows the renamed observations as upx does"""
        self.counts = np.zeros((self.n, 4), dtype=np.int32)
        follow = self.mode == "follow"
        for s in range(self.n):
            p = np.asarray(pairs[s], dtype=np.int64).reshape(-1, 2)
            if len(p) == 0:
                continue
            m = self.m[s]
            shadows = {}
            for name, arr in m.views.items():                    # np_kfmap_merge on a copy of the map whose pixels are the view
                sh = copy.deepcopy(m)
                sh.upx = arr.copy()
                nm.merge(sh, p, None, with_list=follow)
                shadows[name] = sh
            before = {a: m.entry(a) is not None for a in (int(v) for v in p[:, 0])}
            if self.kind == "rows":
                r = nr.merge(m, self.D[s], p, self.lists[s] if follow else None, with_list=follow, log=self.log[s])
            else:
                r = nm.merge(m, p, self.lists[s] if follow else None, with_list=follow, log=self.log[s])
            for name, sh in shadows.items():
                assert np.array_equal(sh.ids, m.ids) and np.array_equal(sh.n, m.n)
                m.views[name] = sh.upx
            if follow and self.lists[s] is not None:
                self.lists[s] = r["list"]
            for a, b in ((int(a), int(b)) for a, b in p):
                if before[a] and m.entry(a) is None:
                    self.ren[s][a] = b
            self.counts[s] = (r["applied"], r["skipped"], r["renamed"], r["status"])
        return self.counts

    def ba(self):
        if self.kind != "rows":
            return super().ba()
        import kfmap_scripts as scr
        out = {}
        for s in range(self.n):
            if not self.sel[s]:
                continue
            win = nr.gather(self.m[s], self.D[s])
            if win is None:
                continue
            theta, outl = scr.refined(self.seeds[s], win), scr.outlier_pattern(self.seeds[s], win)
            lst = nr.update(self.m[s], self.D[s], win, theta, outl, self.lists[s] if self.mode == "follow" else None)
            if lst is not None:
                self.lists[s] = lst
            out[s] = (win, theta, outl)
        return out

    def pixels(self, s, kfid, view="raw"):
        """what KeyframeMap.keyframe_pixels returns for key-frame kfid of stream s, or None"""
        b = self.m[s].slot(kfid)
        return None if b is None else self.m[s].views[view][b, :int(self.m[s].n[b])].copy()


def pairs_of(res):
    return [r["pairs"] if r["status"] == 0 else EMPTY for r in res]


def run_sequence(run, merges=False, on_step=None, **match_kw):
    """kfmap_lmm_scripts' sequence: every key-frame add -> match (-> merge of the match's pairs); a local-BA update behind key-frames 3 and 4; the last
    key-frame without stream 1.  on_step(kind, k, data) after every step ("add", "match", "merge", "ba")."""
    for k in range(ls.N_KF):
        took = run.add(ls.LAST_MASK if k == ls.N_KF - 1 else None)
        on_step and on_step("add", k, took)
        res = run.match(**match_kw)
        on_step and on_step("match", k, res)
        if merges:
            run.merge(pairs_of(res))
            on_step and on_step("merge", k, pairs_of(res))
        if k in ls.BA_AT:
            sol = run.ba()
            on_step and on_step("ba", k, sol)
