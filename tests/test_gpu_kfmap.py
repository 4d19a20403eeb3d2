"""GPU: the key-frame map on the device (slam_kfmap, csrc/kfmap.hip) against the bounded model (tests/np_kfmap.py) on the scripted key-frame
sequences of tests/kfmap_scripts.py: S = 3, cap = 100 (no multiple of 64), min_cov_score 6 .. 12, lists of 0, 1, 63, 64, 65 and cap keypoints.
The same lists go through ks.upload + km.add_keyframe and through the model; read-backs, gathered windows, statuses and, after update, the map
and the live lists are compared.  Bars: everything that is an id, a flag, a set or a copy is array_equal; undistorted pixels within 1e-9 px (what
the frame-statistics tests grant undistort_px); the angles of a key-frame's theta within 1e-12 (what tests/test_pose_records_host.py holds
pose_to_angles to), its translation exact.  Every test fails without the slam_kfmap_* symbols."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_scripts as scr  # noqa: E402
import np_kfmap as npk  # noqa: E402

pytestmark = pytest.mark.gpu
S = 3
PX_TOL, ANGLE_TOL = 1e-9, 1e-12


def _px_same(a, b, exact):
    return a.shape == b.shape and (np.array_equal(a, b) if exact else bool(np.all(np.abs(a - b) <= PX_TOL)))


def _theta_same(a, b, exact):
    return np.array_equal(a[3:], b[3:]) and (np.array_equal(a[:3], b[:3]) if exact else bool(np.all(np.abs(a[:3] - b[:3]) <= ANGLE_TOL)))


class Pair:
    """A device map with its keypoint set, and the model of every stream, driven by one scenario.  step() consumes the next scripted key-frame of
    every selected stream on both sides."""

    def __init__(self, slam, name):
        self.slam = slam
        self.sc, self.frames = scr.scenario(name)
        self.ks = slam.KeypointSet(S, scr.CAP)
        self.km = slam.KeyframeMap(S, scr.CAP, R=self.sc["R"], mcap=self.sc["mcap"])
        self.m = [npk.Map(scr.CAP, self.sc["R"], self.sc["mcap"], scr.CAM, self.sc["dists"][s], self.sc["minc"][s]) for s in range(S)]
        self.nkf = [0] * S                                       # key-frames consumed per stream = the id of its next one
        self.dist = np.array([d if d is not None else (0.0,) * 4 for d in self.sc["dists"]])
        self.Tcw = np.tile(np.eye(4), (S, 1, 1))
        self.sel = [True] * S

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
        sp = self.slam.stream_params(S, Tcw=self.Tcw, cam=scr.CAM, dist=self.dist)
        with self.ks.selected(mask):
            self.ks.keyframe()
            self.km.add_keyframe(self.ks, sp)

    def gather(self, **caps):
        wins, status = self.km.gather(np.array(self.sc["minc"], dtype=np.int32), **caps)
        wm = [npk.gather(self.m[s]) if self.sel[s] else None for s in range(S)]
        return wins, status, wm

    def solution(self, wm):
        """per stream with a model window: the stand-in theta and the hashed outlier flags, the same arrays for both sides"""
        return {s: (scr.refined(self.sc["seeds"][s], w), scr.outlier_pattern(self.sc["seeds"][s], w)) for s, w in enumerate(wm) if w is not None}

    def update(self, wins, wm, sol, follow=True):
        lists = [self.ks.download(s) for s in range(S)]
        self.km.update(wins, [sol[w.stream][0] for w in wins], [sol[w.stream][1] for w in wins], ks=self.ks if follow else None)
        out = list(lists)
        for w in wins:
            s = w.stream
            out[s] = npk.update(self.m[s], wm[s], sol[s][0], sol[s][1], lst=lists[s])
        return out if follow else lists

    # ---- comparisons ----
    def check_windows(self, wins, status, wm):
        want = [3 if not self.sel[s] else (0 if wm[s] is not None else 1) for s in range(S)]
        assert list(status) == want
        assert [w.stream for w in wins] == [s for s in range(S) if want[s] == 0]
        for w in wins:
            self.check_window(w, wm[w.stream])

    def check_window(self, w, ref):
        exact = self.sc["dists"][w.stream] is None
        c, P = w.cache, len(ref["poses_remap"])
        for a, b in ((c.theta_const, ref["theta_const"]), (c.poses_ids, ref["poses_ids"]), (c.points_ids, ref["points_ids"]), (w.poses_remap, ref["poses_remap"]),
                     (w.points_remap, ref["points_remap"]), (w.obs_kf, ref["obs_kf"]), (w.obs_kp, ref["obs_kp"]), (w.obs_in_covmap, ref["obs_in_covmap"])):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert c.poses_ids.dtype == np.int64 and c.poses_ids.min() >= 1 and c.points_ids.min() >= 1
        assert _px_same(c.pixels, ref["pixels"], exact)
        assert len(c.theta) == len(ref["theta"]) and np.array_equal(c.theta[6 * P:], ref["theta"][6 * P:])
        for p in range(P):
            assert _theta_same(c.theta[6 * p:6 * p + 6], ref["theta"][6 * p:6 * p + 6], False)

    def check_state(self, streams=None, exact_kfs=()):
        """the read-backs of the device map against the model; exact_kfs: (stream, kfid) whose theta an update has written (a copy)"""
        for s in (range(S) if streams is None else streams):
            m, exact = self.m[s], self.sc["dists"][s] is None
            for kfid in range(max(self.nkf[s], 1) + 1):
                d, r = self.km.download_keyframe(s, kfid), m.keyframe(kfid)
                assert (d is None) == (r is None), (s, kfid)
                if r is None:
                    continue
                assert np.array_equal(d["ids"], r["ids"]) and np.array_equal(d["live"], r["live"]), (s, kfid)
                assert _px_same(d["upx"], r["upx"], exact) and _theta_same(d["theta"], r["theta"], (s, kfid) in exact_kfs), (s, kfid)
            d, r = self.km.download_points(s), m.points()
            assert np.array_equal(d["ids"], r["ids"]) and np.array_equal(d["xyz"], r["xyz"]) and d["observers"] == r["observers"], s
            for k in ("is_3d", "observed", "ba", "gone"):
                assert np.array_equal(d[k], r[k]), (s, k)

    def check_lists(self, want):
        for s in range(S):
            got = self.ks.download(s)
            for k in ("ids", "yx", "is_3d", "xyz"):
                assert np.array_equal(got[k], want[s][k]), (s, k)


def _snapshot(p, s):
    """everything the host can read of stream s's map and list, as bytes"""
    out = [p.km.download_points(s), p.ks.download(s)]
    out += [p.km.download_keyframe(s, k) for k in range(p.nkf[s] + 1)]
    return repr([(sorted((k, np.asarray(v).tobytes() if not isinstance(v, list) else repr(v)) for k, v in d.items()) if d is not None else None) for d in out])


@pytest.fixture()
def pair(slam):
    made = []

    def make(name):
        made.append(Pair(slam, name))
        return made[-1]
    yield make
    for p in made:
        p.close()


@pytest.mark.parametrize("name", ["plain", "ring", "table"])
def test_scripted_sequences_equal_the_model(pair, name):
    p = pair(name)
    sizes = set()
    n_win = 0
    for k in range(len(p.frames[0])):
        p.add()
        sizes |= {len(p.frames[s][k]["ids"]) for s in range(S)}
        p.check_state()
        wins, status, wm = p.gather()
        p.check_windows(wins, status, wm)
        p.check_state()                                          # (the gather demotes is_bad points and clears dangling observers: the map follows)
        sol = p.solution(wm)
        lists = p.update(wins, wm, sol)
        p.check_state(exact_kfs={(w.stream, int(kf)) for w in wins for kf in w.poses_remap})
        p.check_lists(lists)
        n_win += len(wins)
    assert {0, 1, 63, 64, 65, scr.CAP} <= sizes and n_win >= 12


def test_selection_leaves_unselected_streams_alone_and_selected_ones_independent(pair):
    ref = pair("plain")
    windows = {}
    for k in range(5):
        ref.add()
        wins, status, wm = ref.gather()
        for w in wins:
            windows[(w.stream, k)] = w
        ref.update(wins, wm, ref.solution(wm))
    p = pair("plain")
    masks = [(1, 1, 1), (1, 0, 1), (0, 1, 1), (1, 1, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1), (0, 1, 0), (1, 1, 0)]
    n_cmp = 0
    for mask in masks:
        if any(mask[s] and p.nkf[s] >= 5 for s in range(S)):
            break
        before = [_snapshot(p, s) for s in range(S)]
        p.add(mask)
        wins, status, wm = p.gather()
        p.check_windows(wins, status, wm)
        lists = p.update(wins, wm, p.solution(wm))
        p.check_lists(lists)
        for s in range(S):
            if not mask[s]:
                assert _snapshot(p, s) == before[s], s           # byte for byte through add_keyframe, gather and update
        for w in wins:                                           # the same window whoever else was selected
            r = windows[(w.stream, p.nkf[w.stream] - 1)]
            for a, b in ((w.cache.theta, r.cache.theta), (w.cache.pixels, r.cache.pixels), (w.cache.poses_ids, r.cache.poses_ids), (w.cache.points_ids, r.cache.points_ids),
                         (w.cache.theta_const, r.cache.theta_const), (w.obs_kf, r.obs_kf), (w.obs_kp, r.obs_kp), (w.points_remap, r.points_remap)):
                assert np.array_equal(a, b)
            n_cmp += 1
        p.check_state()
    assert n_cmp >= 6


def _scan(sizes, cap_obs):
    """the header's rule: windows in stream order, one that does not fit what is left takes nothing"""
    used, st = 0, []
    for o in sizes:
        st.append(0 if used + o <= cap_obs else 2)
        used += o if st[-1] == 0 else 0
    return st


def test_a_window_that_does_not_fit_leaves_the_others_intact(pair):
    p = pair("plain")
    cap = None
    for k in range(5):                                           # the first key-frame at which three windows exist and a later one is smaller than an earlier one
        p.add()
        wins, status, wm = p.gather()
        O = [len(w.cache.poses_ids) for w in wins]
        cap = next((c for c in range(sum(O)) if len(wins) == 3 and 2 in _scan(O, c) and 0 in _scan(O, c)[_scan(O, c).index(2):]), None)      # a 2 with a 0 behind it
        if cap is not None:
            break
        p.update(wins, wm, p.solution(wm))
    assert cap is not None
    want = _scan(O, cap)
    small, status = p.km.gather(np.array(p.sc["minc"], dtype=np.int32), max_obs=cap)
    assert list(status) == want
    assert [w.stream for w in small] == [s for s in range(S) if want[s] == 0]
    for w in small:
        r = wins[w.stream]
        for a, b in ((w.cache.theta, r.cache.theta), (w.cache.pixels, r.cache.pixels), (w.cache.poses_ids, r.cache.poses_ids), (w.cache.points_ids, r.cache.points_ids),
                     (w.cache.theta_const, r.cache.theta_const), (w.obs_kf, r.obs_kf), (w.obs_kp, r.obs_kp), (w.obs_in_covmap, r.obs_in_covmap),
                     (w.poses_remap, r.poses_remap), (w.points_remap, r.points_remap)):
            assert np.array_equal(a, b)
    # the window that did not fit is not pending
    with pytest.raises(p.slam.SlamHipError, match="no pending window"):
        p.km.update([want.index(2)], [np.zeros(1)], [np.zeros(1)])


def test_update_without_a_pending_window_fails_and_enqueues_nothing(pair):
    p = pair("plain")
    for k in range(3):
        p.add()
        wins, status, wm = p.gather()
        if k < 2:
            p.update(wins, wm, p.solution(wm))
    assert len(wins) >= 2
    sol = p.solution(wm)
    first = wins[0]
    p.update([first], wm, sol)                                   # consumes stream first.stream's window
    p.check_state(exact_kfs={(first.stream, int(kf)) for kf in first.poses_remap})
    before = [_snapshot(p, s) for s in range(S)]
    rest = [w for w in wins if w is not first]
    with pytest.raises(p.slam.SlamHipError, match="no pending window"):      # one stream with a window, one without: nothing happens to either
        p.km.update(rest + [first], [sol[w.stream][0] for w in rest + [first]], [sol[w.stream][1] for w in rest + [first]], ks=p.ks)
    assert [_snapshot(p, s) for s in range(S)] == before
    lists = p.update(rest, wm, sol)                              # ... and the other windows are still pending
    p.check_state(exact_kfs={(w.stream, int(kf)) for w in wins for kf in w.poses_remap})
    p.check_lists(lists)


@pytest.mark.parametrize("name,later", [("plain", 1), ("ring", 1), ("ring", 2)])
def test_update_after_later_keyframes(pair, name, later):
    """the window of key-frame 4 applied after `later` more key-frames; in the ring of 4 the first of them takes the slot of key-frame 1, one of the window's"""
    p = pair(name)
    for k in range(5):
        p.add()
        wins, status, wm = p.gather()
        if k < 4:
            p.update(wins, wm, p.solution(wm))
    sol = p.solution(wm)
    if name == "ring":
        assert any(int(kf) <= later for w in wins for kf in w.poses_remap), "a key-frame of a window is about to be forgotten"
    for _ in range(later):
        p.add()
    p.check_state()
    lists = p.update(wins, wm, sol)
    p.check_state(exact_kfs={(w.stream, int(kf)) for w in wins for kf in w.poses_remap})
    p.check_lists(lists)


def test_gathered_windows_solve_like_the_models(pair):
    p = pair("plain")
    slam = p.slam
    for k in range(5):
        p.add()
        wins, status, wm = p.gather()
        if k < 4:
            p.update(wins, wm, p.solution(wm))
    assert len(wins) == 3
    ref = [slam.LocalBACache(wm[w.stream]["theta"].copy(), wm[w.stream]["theta_const"], wm[w.stream]["pixels"], wm[w.stream]["poses_ids"], wm[w.stream]["points_ids"])
           for w in wins]
    st_d = slam.bundle_adjustment_batch_([w.cache for w in wins], scr.CAM)
    st_r = slam.bundle_adjustment_batch_(ref, scr.CAM)
    assert np.array_equal(st_d, st_r) and not st_d.any()
    for w, r in zip(wins, ref):
        assert np.array_equal(w.cache.outliers, r.outliers)
        assert np.allclose(w.cache.theta, r.theta, rtol=1e-6, atol=1e-9)
        assert w.cache.stats["ssr_final"] < w.cache.stats["ssr_init"]
