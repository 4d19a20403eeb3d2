"""GPU: slam_kfmap_filter / slam_kfmap_remove_keyframe (csrc/kfmap.hip) against the bounded model (tests/np_kfmap_filter.py over tests/np_kfmap.py)
on the scripted case of np_kfmap_filter.STREAMS: S = 4 (the fourth stream's ratio is 1.0: it must stay untouched), cap 100, min_cov_score 8,
first_kfid 6; after each key-frame gather -> update -> filter on both sides.

Comparison: the `removed` words, every key-frame of the ring (download_keyframe for ALL ids so far, None where removed or forgotten) and
download_points, array_equal to the model after every step.  One number of the map is computed on the device in its own arithmetic -- a
key-frame's RotZYX angles (pose_to_angles; held to 1e-12 by tests/test_gpu_kfmap.py); add() checks them to that bar once and hands the device's
bits to the model, so that every later comparison, thetas included, is array_equal.  Every test fails without the slam_kfmap_filter symbol."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_scripts as scr  # noqa: E402
import np_kfmap as npk  # noqa: E402
import np_kfmap_filter as flt  # noqa: E402

pytestmark = pytest.mark.gpu
S = 4
ANGLE_TOL = 1e-12


class Rig:
    """A device map with its keypoint set and the model of every stream; every step runs on both sides"""

    def __init__(self, slam, R, frames=None, cap=flt.CAP, ratios=None, minc=flt.MINC, first=flt.FIRST):
        self.slam, self.R, self.cap = slam, R, cap
        self.frames = frames if frames is not None else [flt.frames(cfg) for cfg in flt.STREAMS]
        self.ratios = np.array(ratios if ratios is not None else [cfg["ratio"] for cfg in flt.STREAMS], dtype=np.float64)
        self.minc, self.first = np.full(S, minc, dtype=np.int32), first
        self.ks = slam.KeypointSet(S, cap)
        self.km = slam.KeyframeMap(S, cap, R=R, mcap=flt.MCAP)
        self.m = [npk.Map(cap, R, flt.MCAP, scr.CAM, None, minc) for _ in range(S)]
        self.nkf = [0] * S
        self.Tcw = np.tile(np.eye(4), (S, 1, 1))
        self.sel = [True] * S
        self.logs = []                                           # (stream, key-frame, model log) of every filter

    def close(self):
        self.km.close(); self.ks.close()

    def add(self, mask=None):
        self.sel = [True] * S if mask is None else [bool(v) for v in mask]
        for s in range(S):
            if self.sel[s]:
                f = self.frames[s][self.nkf[s]]
                self.ks.upload(s, f["yx"], f["is_3d"], f["xyz"], f["ids"])
                self.Tcw[s] = f["Tcw"]
                npk.add_keyframe(self.m[s], self.nkf[s], f["Tcw"], f)
                self.nkf[s] += 1
        sp = self.slam.stream_params(S, Tcw=self.Tcw, cam=scr.CAM, dist=np.zeros((S, 4)))
        with self.ks.selected(mask):
            self.ks.keyframe()
            self.km.add_keyframe(self.ks, sp)
        for s in range(S):                                       # the device's angles, checked to their bar, become the model's
            if self.sel[s]:
                k = self.nkf[s] - 1
                th, ref = self.km.download_keyframe(s, k)["theta"], self.m[s].theta[k % self.R]
                assert np.array_equal(th[3:], ref[3:]) and np.all(np.abs(th[:3] - ref[:3]) <= ANGLE_TOL), (s, k)
                self.m[s].theta[k % self.R] = th

    def gather(self):
        wins, status = self.km.gather(self.minc)
        wm = [npk.gather(self.m[s]) if self.sel[s] else None for s in range(S)]
        assert [w.stream for w in wins] == [s for s in range(S) if wm[s] is not None]
        for w in wins:
            assert np.array_equal(w.cache.theta, wm[w.stream]["theta"]) and np.array_equal(w.obs_kp, wm[w.stream]["obs_kp"])
        seeds = [cfg["seed"] for cfg in flt.STREAMS]
        sol = {s: (scr.refined(seeds[s], w), scr.outlier_pattern(seeds[s], w)) for s, w in enumerate(wm) if w is not None}
        return wins, wm, sol

    def update(self, wins, wm, sol):
        self.km.update(wins, [sol[w.stream][0] for w in wins], [sol[w.stream][1] for w in wins], ks=None)
        for w in wins:
            npk.update(self.m[w.stream], wm[w.stream], sol[w.stream][0], sol[w.stream][1])

    def filter(self, want_removed=True):
        got = self.km.filter(self.ratios, self.minc, first_kfid=self.first, want_removed=want_removed)
        want = []
        for s in range(S):
            log = flt.filter_map(self.m[s], float(self.ratios[s]), int(self.minc[s]), self.first) if self.sel[s] else []
            self.logs.append((s, self.nkf[s] - 1, log))
            want.append(sorted(k for k, ex, _, _ in log if ex in ("few", "ratio")))
        if want_removed:
            assert got == want, (got, want)
            assert [int(w) for w in self.km.last_removed_masks] == [flt.removed_mask(self.logs[-S + s][2], self.R) for s in range(S)]
        else:
            assert got is None
        return want

    def check_state(self, streams=None):
        for s in (range(S) if streams is None else streams):
            m = self.m[s]
            for kfid in range(self.nkf[s] + 1):
                d, r = self.km.download_keyframe(s, kfid), m.keyframe(kfid)
                assert (d is None) == (r is None), (s, kfid)
                if r is not None:
                    for k in ("theta", "ids", "upx", "live"):
                        assert np.array_equal(d[k], r[k]), (s, kfid, k)
            d, r = self.km.download_points(s), m.points()
            assert np.array_equal(d["ids"], r["ids"]) and np.array_equal(d["xyz"], r["xyz"]) and d["observers"] == r["observers"], s
            for k in ("is_3d", "observed", "ba", "gone"):
                assert np.array_equal(d[k], r[k]), (s, k)

    def step(self, mask=None, want_removed=True, check=True):
        self.add(mask)
        wins, wm, sol = self.gather()
        self.update(wins, wm, sol)
        if check:
            self.check_state()
        removed = self.filter(want_removed)
        if check:
            self.check_state()
        return removed

    def snapshot(self, s):
        """everything the host can read of stream s's map, as bytes"""
        out = [self.km.download_points(s)] + [self.km.download_keyframe(s, k) for k in range(len(self.frames[s]) + 1)]
        return repr([(sorted((k, np.asarray(v).tobytes() if not isinstance(v, list) else repr(v)) for k, v in d.items()) if d is not None else None) for d in out])

    def exits(self):
        return {ex for _, _, log in self.logs for _, ex, _, _ in log}


@pytest.fixture()
def rig(slam):
    made = []

    def make(*a, **k):
        made.append(Rig(slam, *a, **k))
        return made[-1]
    yield make
    for p in made:
        p.close()


@pytest.mark.parametrize("R", [8, 16])
def test_scripted_case_equals_the_model(rig, R):
    p = rig(R)
    removed = [[] for _ in range(S)]
    for k in range(len(flt.SIZES)):
        for s, ids in enumerate(p.step()):
            removed[s] += ids
    assert removed[3] == [] and sum(len(r) for r in removed) >= 2
    if R == 8:                                                   # the coverage tests/test_kfmap_filter_host.py asserts of the model holds for this run too
        assert p.exits() == {"break", "keep", "few", "ratio"}
        assert any(ex == "keep" and t and g / t == flt.STREAMS[s]["ratio"] for s, _, log in p.logs for _, ex, t, g in log)
        assert 3 in removed[0] and p.nkf[0] > 11                 # slot 3 of stream A was emptied, then key-frame 11 was recorded into it


def _edge_frames():
    """cap 300: the key-frames hold ids 1 .. n (nested: a point's observers are the key-frames at least that long), so the candidates of the
    newest key-frame are slabs of 1, 255, 256, 257 and 300 observations -- the chunk edges of k_kfm_filter -- beside an empty slab (key-frame 6;
    a slab without an observation shares no point and cannot be a candidate itself) and key-frame 0, which sees a point of its own."""
    sizes = (1, 1, 255, 256, 257, 300, 0, 300)
    frames = []
    for s in range(S):
        fr = []
        for k, n in enumerate(sizes):
            ids = np.array([0], dtype=np.int64) if k == 0 else np.arange(1, n + 1, dtype=np.int64)
            n = len(ids)
            f3 = np.array([scr._u(77 + s, 1, int(i)) < (0.5 + 0.1 * s) or int(i) == 1 for i in ids], dtype=bool)     # is_3d is a function of the id
            xyz = np.array([scr.world_point(77 + s, int(i)) for i in ids]).reshape(-1, 3)
            yx = np.array([[10.0 + 0.5 * int(i), 20.0 + 0.25 * int(i) + k] for i in ids]).reshape(-1, 2)
            fr.append(dict(Tcw=scr.pose(77 + s, k), ids=ids, yx=yx, is_3d=f3, xyz=xyz))
        frames.append(fr)
    return sizes, frames


def test_chunk_edges(rig):
    sizes, frames = _edge_frames()
    p = rig(8, frames=frames, cap=300, ratios=(0.97, 0.99, 0.5, 1.0), minc=4, first=7)
    for k in range(len(sizes)):
        p.add()
        p.check_state()
        removed = p.filter()
        p.check_state()
    walked = {len(frames[s][kfid]["ids"]) for s, _, log in p.logs for kfid, ex, _, _ in log if ex != "break"}      # the lengths of the slabs the phases walked
    assert {1, 255, 256, 257, 300} <= walked, walked
    assert {"keep", "few", "ratio"} <= p.exits() and removed[3] == [], (p.exits(), removed)


def test_selection_leaves_the_other_streams_alone(rig):
    p = rig(8)
    for k in range(8):
        p.step(check=False)
    p.check_state()
    for mask in ((1, 0, 1, 0), (0, 1, 0, 1), (0, 0, 1, 0)):      # key-frames 8, 8, 9: the filters that remove
        before = [p.snapshot(s) for s in range(S)]
        removed = p.step(mask)
        for s in range(S):
            if not mask[s]:
                assert removed[s] == [] and p.snapshot(s) == before[s], s
    assert sum(ex in ("few", "ratio") for _, _, log in p.logs for _, ex, _, _ in log) >= 3


def test_filter_between_gather_and_update(rig):
    p = rig(8)
    for k in range(8):
        p.step(check=False)
    p.add()
    wins, wm, sol = p.gather()
    removed = p.filter()
    p.check_state()
    # a key-frame the filter removed is a pose of the pending window and has outlier observations inside the covisibility map (stream C's key-frame 7)
    hit = [(s, k) for s in range(S) for k in removed[s] if wm[s] is not None and k in wm[s]["poses_remap"]
           and (sol[s][1] & wm[s]["obs_in_covmap"] & (wm[s]["obs_kf"] == k)).any()]
    assert hit
    p.update(wins, wm, sol)
    p.check_state()
    for k in range(9, 12):
        p.step()


def test_remove_keyframe_equals_the_model(rig):
    p = rig(8)
    for k in range(5):
        p.step(check=False)
    p.check_state()
    for s, kfid in ((0, 2), (1, 0), (2, 3), (0, 2), (3, 9), (1, 12)):      # ... again (no longer there), never added, beyond the ring
        p.km.remove_keyframe(s, kfid)
        flt.remove_keyframe(p.m[s], kfid)
        p.check_state()
    before = [p.snapshot(s) for s in range(S)]
    with pytest.raises(p.slam.SlamHipError, match="newest"):
        p.km.remove_keyframe(2, 4)
    with pytest.raises(ValueError):
        flt.remove_keyframe(p.m[2], 4)
    assert [p.snapshot(s) for s in range(S)] == before
    for k in range(5, 10):                                       # the emptied slots take part in gathers and are recorded into (key-frame 8 -> slot 0)
        p.step()


def test_argument_errors_enqueue_nothing(rig):
    p = rig(8)
    for k in range(8):
        p.step(check=False)
    p.add()
    before = [p.snapshot(s) for s in range(S)]
    for ratios, minc, first in (((0.5, float("nan"), 0.7, 1.0), p.minc, 6), ((0.5, 0.6, float("-inf"), 1.0), p.minc, 6),
                                (p.ratios, np.array([8, 8, 8, -1], dtype=np.int32), 6), (p.ratios, p.minc, -1)):
        for want in (True, False):
            with pytest.raises(p.slam.SlamHipError):
                p.km.filter(ratios, minc, first_kfid=first, want_removed=want)
    assert [p.snapshot(s) for s in range(S)] == before
    p.ratios = np.array([0.5, float("inf"), 2.0, 1.0])           # legal: at or above 1 the filter does not act
    removed = p.filter()
    assert removed[0] and removed[1:] == [[], [], []]
    p.check_state()


def test_the_same_sequence_twice_gives_identical_bytes_with_or_without_the_read_back(rig):
    a, b, c = rig(8), rig(8), rig(8)
    for k in range(10):
        a.step(check=False)
        b.step(check=False)
        c.step(check=False, want_removed=k == 9)                 # enqueue-only filters, then one synchronous call
    c.check_state()
    sa = [a.snapshot(s) for s in range(S)]
    assert sa == [b.snapshot(s) for s in range(S)] and sa == [c.snapshot(s) for s in range(S)]
