"""GPU: KeyframeMap.local_ba (slam_kfmap_local_ba) -- the estimator step with the windows resident in HBM -- against the host route on a second map
driven by the same script (tests/kfmap_scripts.py, S = 3, cap = 100, R = 4 and 8): map A takes gather -> bundle_adjustment_batch_ -> update(ks), map
B takes local_ba(ks).  After every step the downloads of key-frames, points and live lists are compared: every discrete field array_equal (ids, masks,
flags, live, list lengths, what was removed), positions and theta to 1e-6 relative (the contract of the two solve routes).  For the outlier sets to be
comparable, every window is asserted to keep its squared residuals 1e-3 relative away from repr_eps and its depths from 1e-6 at the pass-1 theta
(test_gpu_ba_batch_dev's precondition)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_scripts as scr  # noqa: E402
import test_gpu_ba_batch_dev as tbd  # noqa: E402

pytestmark = pytest.mark.gpu
S = 3
REL = 1e-6


class Side:
    def __init__(self, slam, sc):
        self.ks = slam.KeypointSet(S, scr.CAP)
        self.km = slam.KeyframeMap(S, scr.CAP, R=sc["R"], mcap=sc["mcap"])

    def close(self):
        self.km.close(); self.ks.close()


class Two:
    """two maps with their keypoint sets, fed the same scripted key-frames"""

    def __init__(self, slam, name, minc=None):
        self.slam = slam
        self.sc, self.frames = scr.scenario(name)
        self.minc = np.array(self.sc["minc"] if minc is None else minc, dtype=np.int32)
        self.a, self.b = Side(slam, self.sc), Side(slam, self.sc)
        self.nkf = [0] * S
        self.dist = np.array([d if d is not None else (0.0,) * 4 for d in self.sc["dists"]])
        self.Tcw = np.tile(np.eye(4), (S, 1, 1))

    def close(self):
        self.a.close(); self.b.close()

    def add(self, mask=None):
        sel = [True] * S if mask is None else [bool(v) for v in mask]
        for s in range(S):
            if sel[s]:
                f = self.frames[s][self.nkf[s]]
                for side in (self.a, self.b):
                    side.ks.upload(s, f["yx"], f["is_3d"], f["xyz"], f["ids"])
                self.Tcw[s] = f["Tcw"]
                self.nkf[s] += 1
        sp = self.slam.stream_params(S, Tcw=self.Tcw, cam=scr.CAM, dist=self.dist)
        for side in (self.a, self.b):
            with side.ks.selected(mask):
                side.ks.keyframe()
                side.km.add_keyframe(side.ks, sp)
        return sel

    def host_step(self):
        """map A: gather -> (precondition) -> bundle_adjustment_batch_ -> update(ks); -> (windows, gather status, batch status)"""
        slam = self.slam
        wins, status = self.a.km.gather(self.minc)
        st = np.zeros(0, dtype=np.int32)
        if wins:
            ws = [dict(P=w.cache.n_poses, M=w.cache.n_points, O=len(w.cache.poses_ids), cam=scr.CAM, theta0=w.cache.theta.copy(), theta_const=w.cache.theta_const,
                       pixels_yx=w.cache.pixels, pose_ids=w.cache.poses_ids, point_ids=w.cache.points_ids) for w in wins]
            tbd._assert_margin(slam, ws)
            st = slam.bundle_adjustment_batch_([w.cache for w in wins], scr.CAM, repr_eps=tbd.REPR_EPS)
            ok = [w for w, c in zip(wins, st) if c == 0]
            if ok:
                self.a.km.update(ok, ks=self.a.ks)
        return wins, status, st

    def compare(self):
        for s in range(S):
            da, db = self.a.km.download_points(s), self.b.km.download_points(s)
            assert np.array_equal(da["ids"], db["ids"]) and da["observers"] == db["observers"], s
            for k in ("is_3d", "observed", "ba", "gone"):
                assert np.array_equal(da[k], db[k]), (s, k)
            assert np.abs(da["xyz"] - db["xyz"]).max(initial=0.0) <= REL * max(1.0, np.abs(da["xyz"]).max(initial=0.0)), s
            for kfid in range(max(self.nkf[s], 1) + 1):
                ka, kb = self.a.km.download_keyframe(s, kfid), self.b.km.download_keyframe(s, kfid)
                assert (ka is None) == (kb is None), (s, kfid)
                if ka is None:
                    continue
                assert np.array_equal(ka["ids"], kb["ids"]) and np.array_equal(ka["live"], kb["live"]) and np.array_equal(ka["upx"], kb["upx"]), (s, kfid)
                assert np.abs(ka["theta"] - kb["theta"]).max() <= REL * max(1.0, np.abs(ka["theta"]).max()), (s, kfid)
            la, lb = self.a.ks.download(s), self.b.ks.download(s)
            assert np.array_equal(la["ids"], lb["ids"]) and np.array_equal(la["is_3d"], lb["is_3d"]) and np.array_equal(la["yx"], lb["yx"]), s
            assert np.abs(la["xyz"] - lb["xyz"]).max(initial=0.0) <= REL * max(1.0, np.abs(la["xyz"]).max(initial=0.0)), s


@pytest.fixture()
def two(slam):
    made = []

    def make(name, **kw):
        made.append(Two(slam, name, **kw))
        return made[-1]
    yield make
    for t in made:
        t.close()


def _step(t, mask=None):
    sel = t.add(mask)
    wins, gstat, bstat = t.host_step()
    status, stats = t.b.km.local_ba(t.minc, scr.CAM, ks=t.b.ks, repr_eps=tbd.REPR_EPS)
    want = gstat.copy()
    for w, c in zip(wins, bstat):
        want[w.stream] = c
    assert status.tolist() == want.tolist(), (status, want)
    pmo = t.b.km.last_windows()
    for w, c in zip(wins, bstat):
        assert pmo[w.stream].tolist() == [w.cache.n_poses, w.cache.n_points, len(w.cache.poses_ids)]
        if c == 0:
            sa = w.cache.stats
            assert int(stats[w.stream][3]) == sa["iters_pass1"] and int(stats[w.stream][4]) == sa["iters_pass2"] and int(stats[w.stream][5]) == sa["n_outliers"]
            assert abs(stats[w.stream][2] - sa["ssr_final"]) <= 1e-8 * max(sa["ssr_final"], 1e-300)
    t.compare()
    # no pending window is left behind: within one call no key-frame can come between plan and apply, so a following update finds nothing to apply
    for w, c in zip(wins, bstat):
        if c == 0:
            with pytest.raises(t.slam.SlamHipError, match="no pending window"):
                t.b.km.update([w.stream], [w.cache.theta], [w.cache.outliers])
    return wins, status


@pytest.mark.parametrize("name", ["ring", "plain"])
def test_local_ba_equals_gather_solve_update(two, name):
    """R = 4 and 8; stream 1 sits out two steps (not selected), stream 2 has no window at first (a list of one keypoint)"""
    t = two(name)
    seen = set()
    for k in range(7):
        mask = [1, 0, 1] if k in (2, 4) else None
        wins, status = _step(t, mask)
        seen |= set(status.tolist())
    assert {0, 1, 3} <= seen, seen


def test_a_window_the_device_batch_does_not_take_goes_through_the_host_route(two, slam):
    """a high min_cov_score leaves a stream's window one free pose (the new key-frame) among several: slam_local_ba_batch_dev refuses it, the call solves
    it through slam_local_ba_batch and the map still matches"""
    t = two("plain", minc=(58, 12, 6))
    one_free = 0
    for k in range(7):
        wins, status = _step(t)
        for w in wins:
            if (w.cache.theta_const == 0).sum() == 1 and w.cache.n_poses > 1 and status[w.stream] == 0:
                one_free += 1
    assert one_free >= 1, "the script never produced a window with one free pose among several"


def test_a_map_that_never_calls_local_ba_launches_what_it_always_did(slam):
    """the spans of the host route's calls are the gather's and the update's alone; local_ba adds the device batch's"""
    ctx = slam.default_context(0)
    sc, frames = scr.scenario("plain")

    def run(device):
        side = Side(slam, sc)
        names = ["kfmap_add", "kfmap_gather_plan", "kfmap_gather_emit", "kfmap_update", "ba_dev_probe", "ba_dev_stage", "ba_dev_results"]
        ctx.prof_enable(True); ctx.prof_reset()
        Tcw = np.tile(np.eye(4), (S, 1, 1))
        for k in range(3):
            for s in range(S):
                f = frames[s][k]
                side.ks.upload(s, f["yx"], f["is_3d"], f["xyz"], f["ids"]); Tcw[s] = f["Tcw"]
            side.ks.keyframe()
            side.km.add_keyframe(side.ks, slam.stream_params(S, Tcw=Tcw, cam=scr.CAM))
            if device:
                side.km.local_ba(np.array(sc["minc"], dtype=np.int32), scr.CAM, ks=side.ks)
            else:
                wins, _ = side.km.gather(np.array(sc["minc"], dtype=np.int32))
                if wins:
                    slam.bundle_adjustment_batch_([w.cache for w in wins], scr.CAM)
                    side.km.update(wins, ks=side.ks)
        ctx.synchronize()
        got = {n: ctx.prof_get(n)[1] for n in names}
        ctx.prof_enable(False)
        side.close()
        return got
    host, dev = run(False), run(True)
    assert host["ba_dev_probe"] == host["ba_dev_stage"] == host["ba_dev_results"] == 0
    assert host["kfmap_gather_plan"] == 3 and host["kfmap_update"] >= 1 and host["kfmap_add"] == 3
    assert dev["kfmap_gather_plan"] == 3 and dev["ba_dev_probe"] >= 1 and dev["kfmap_update"] == host["kfmap_update"] and dev["kfmap_gather_emit"] == host["kfmap_gather_emit"]
