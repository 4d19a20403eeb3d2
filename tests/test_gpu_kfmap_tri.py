"""GPU: slam_kfmap_triangulate_temporal (csrc/kfmap_tri.inc) -- triangulate_temporal! from the map's own key-frames -- against the model
(tests/np_kfmap_tri.py) on the sequences of tests/kfmap_tri_scripts.py (tests/test_kfmap_tri_host.py shows what each holds and that the model equals a
literal restatement of the reference).  For every sequence, after EVERY step:

  * every key-frame of the ring (download_keyframe), download_points and, where the row store is on, descriptor_rows are array_equal to the model in
    ids, live bytes, masks, flags and counts; the live list is equal in ids, yx, is_3d and length;
  * after a triangulation step the call's counts equal the model's, and the accepted positions are within rtol 1e-9, atol 1e-9 of slam.triangulate's
    temporal mode fed with the pairs, parallaxes and rel_pose_inv the model selected, followed by observer.wc in numpy -- the comparison and the
    tolerance of test_temporal_triangulation_on_the_set_equals_the_host_seam; that seam's verdicts equal the model's decisions.  The device's bits
    then become the model's, so that every later comparison, positions included, is array_equal.

(A key-frame's angles are computed on the device in its own arithmetic; add() holds them to 1e-12 once, as the other map tests do, and hands the
device's bits to the model.)  Every test fails without slam_kfmap_triangulate_temporal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_tri_scripts as ts  # noqa: E402
import np_kfmap_rows as nr  # noqa: E402
import np_kfmap_tri as nt  # noqa: E402

pytestmark = pytest.mark.gpu
ANGLE_TOL = 1e-12
DCAP = 320


def device_bytes(km, ks, s, nkf):
    """what can be read back of stream s's share of the allocations, as bytes"""
    d = [km.download_points(s), ks.download(s)] + [km.download_keyframe(s, k) for k in range(nkf)]
    return repr([(sorted((k, np.asarray(v).tobytes() if not isinstance(v, list) else repr(v)) for k, v in x.items()) if x is not None else None) for x in d])


class Dev(ts.TriRun):
    """the device map with its keypoint set beside the models, driven through the same steps"""

    def __init__(self, slam, want_counts=True, **kw):
        import torch
        self.torch, self.slam, self.want_counts = torch, slam, want_counts
        super().__init__(**kw)
        self.ks = slam.KeypointSet(self.S, self.cap)
        self.km = slam.KeyframeMap(self.S, self.cap, R=self.R, mcap=self.mcap)
        if self.rows:
            self.km.enable_descriptors()
            self.km.enable_descriptor_rows(self.rows)
        self.Tcw = np.tile(np.eye(4), (self.S, 1, 1))
        self.dev_wins = None
        self.n_pos = 0

    def close(self):
        self.km.close(); self.ks.close()

    @property
    def kset(self):
        return self.ks if self.with_list else None

    def add(self, mask=None):
        took = super().add(mask)
        S = self.S
        for s, f in took.items():
            self.ks.upload(s, f["yx"], f["is_3d"], f["xyz"], f["ids"])
            self.Tcw[s] = f["Tcw"]
        sp = self.slam.stream_params(S, Tcw=self.Tcw, cam=ts.CAM, dist=np.zeros((S, 4)))
        with self.ks.selected(mask):
            self.ks.keyframe()
            self.km.add_keyframe(self.ks, sp)
            if self.rows:
                desc = np.full((S, DCAP, 4), 0x5555555555555555, dtype=np.uint64)
                info = np.tile(np.array([10 ** 6, 3], dtype=np.int64), (S, 1))
                for s, f in took.items():
                    born = self.tracks[s][self.nkf[s] - 1][1]
                    new = [int(i) for i in f["ids"] if int(i) >= born]
                    if new:
                        rows = self.desc_rows(s, new)
                        info[s] = (new[0], len(rows)); desc[s, :len(rows)] = rows
                desc_dev = self.torch.from_numpy(desc.view(np.int64)).cuda(); info_dev = self.torch.from_numpy(info).cuda()
                self.km.add_descriptors(desc_dev.data_ptr(), info_dev.data_ptr(), DCAP)
                self.km.ctx.synchronize()                        # (the tensors live until the kernel has read them)
        for s in took:                                           # the device's angles, checked to their bar, become the model's
            k = self.nkf[s] - 1
            th, ref = self.km.download_keyframe(s, k)["theta"], self.m[s].theta[k % self.R]
            assert np.array_equal(th[3:], ref[3:]) and np.all(np.abs(th[:3] - ref[:3]) <= ANGLE_TOL), (s, k)
            self.m[s].theta[k % self.R] = th
        return took

    def tri(self, mutant=None, with_list=None):
        want = super().tri(mutant, with_list)
        got = self.km.triangulate_temporal(ts.CAM, ks=self.kset, max_error=ts.MAX_ERROR, min_depth=ts.MIN_DEPTH, min_parallax=ts.MIN_PARALLAX,
                                           want_counts=self.want_counts)
        assert (got is None) == (not self.want_counts)
        for s, r in enumerate(want):
            if got is not None:
                assert np.array_equal(got[s], r["counts"] if r is not None else np.zeros(4, dtype=np.int32)), (s, got[s], None if r is None else r["counts"])
            if r is None:
                continue
            # the host seam on the pairs the model selected, per observer key-frame: its verdicts are the model's decisions, its points the device's
            pts = self.km.download_points(s)
            at = {int(i): j for j, i in enumerate(pts["ids"])}
            paired = [c for c in r["cand"] if c["code"] in (nt.ACCEPTED, nt.REMOVED)]
            for ob in sorted(set(c["observer"] for c in paired)):
                grp = [c for c in paired if c["observer"] == ob]
                Xc, ok = self.slam.triangulate(ts.CAM, ts.CAM, grp[0]["rel_inv"], np.array([c["obup"] for c in grp]), np.array([c["kpup"] for c in grp]),
                                               ts.MAX_ERROR, min_depth=ts.MIN_DEPTH, parallax=np.array([c["parallax"] for c in grp]), min_parallax=ts.MIN_PARALLAX)
                assert [bool(v) for v in ok] == [c["code"] == nt.ACCEPTED for c in grp], (s, ob)
                wob = grp[0]["wob"]
                for c, X in zip(grp, Xc @ wob[:3, :3].T + wob[:3, 3]):
                    if c["code"] != nt.ACCEPTED:
                        continue
                    dev = pts["xyz"][at[c["id"]]]
                    assert np.allclose(dev, X, rtol=1e-9, atol=1e-9), (s, c["id"], np.abs(dev - X).max())
                    assert np.allclose(dev, c["xyz"], rtol=1e-9, atol=1e-9), (s, c["id"])
                    self.m[s].xyz[c["id"] % self.mcap] = dev; c["xyz"] = dev.copy()          # the device's bits become the model's
                    if self.with_list:
                        hit = np.flatnonzero(self.lists[s]["ids"] == c["id"])
                        if len(hit):
                            self.lists[s]["xyz"][hit[0]] = dev
                    self.n_pos += 1
        return want

    def remove_keyframe(self, s, kfid):
        super().remove_keyframe(s, kfid)
        self.km.remove_keyframe(s, kfid)

    def gather(self):
        want = super().gather()
        wins, status = self.km.gather(np.full(self.S, self.minc, dtype=np.int32))
        assert [w.stream for w in wins] == sorted(want)
        for w in wins:                                           # the gather searched the slabs the triangulation wrote: the window is the model's
            ref = want[w.stream]
            assert np.array_equal(w.cache.theta, ref["theta"]) and np.array_equal(w.cache.pixels, ref["pixels"])
            assert np.array_equal(w.obs_kf, ref["obs_kf"]) and np.array_equal(w.obs_kp, ref["obs_kp"]) and np.array_equal(w.points_remap, ref["points_remap"])
        self.dev_wins = wins
        return want

    def update(self, wins, sols):
        super().update(wins, sols)
        self.km.update(self.dev_wins, [sols[w.stream][0] for w in self.dev_wins], [sols[w.stream][1] for w in self.dev_wins], ks=self.kset)

    def merge(self, pairs):
        want = super().merge(pairs)
        got = self.km.merge(self.kset, [np.asarray(p, dtype=np.int64).reshape(-1, 2) for p in pairs])
        assert np.array_equal(got, want), (got, want)
        return want

    def check(self):
        for s, m in enumerate(self.m):
            for k in range(max(m.cur - self.R + 1, 0), m.cur + 1):
                d, w = self.km.download_keyframe(s, k), m.keyframe(k)
                assert (d is None) == (w is None), (s, k)
                if w is not None:
                    assert all(np.array_equal(d[key], w[key]) for key in ("theta", "ids", "upx", "live")), (s, k)
            d, w = self.km.download_points(s), m.points()
            assert all(np.array_equal(d[key], w[key]) for key in ("ids", "xyz", "is_3d", "observed", "ba", "gone")) and d["observers"] == w["observers"], s
            if self.lists[s] is not None:
                d = self.ks.download(s)
                assert len(d["ids"]) == len(self.lists[s]["ids"]) and all(np.array_equal(d[key], self.lists[s][key]) for key in ("ids", "yx", "is_3d", "xyz")), s
            if self.rows:
                assert nr.same_rows(self.km.descriptor_rows(s), nr.descriptor_rows(m, self.D[s])), s


@pytest.fixture()
def dev(slam):
    made = []

    def make(name, **kw):
        run, fn = ts.make(name, cls=lambda **a: Dev(slam, **a), **kw)
        made.append(run)
        return run, fn
    yield make
    for p in made:
        p.close()


@pytest.mark.parametrize("name", sorted(ts.SEQUENCES))
def test_device_equals_model_after_every_step(dev, slam, name):
    run, fn = dev(name)
    seen = dict(steps=0, before=None)

    def on_step(step):
        run.check()
        seen["steps"] += 1
        if name == "selection" and step == "add2":                # 7: the unselected stream's bytes, before the call
            seen["before"] = device_bytes(run.km, run.ks, 1, run.nkf[1])
        if name == "selection" and step == "tri2":
            assert device_bytes(run.km, run.ks, 1, run.nkf[1]) == seen["before"] and run.last[1] is None
    run.on_step = on_step
    if name == "no_rows":                                        # 9: a map that never enables rows launches <false>: the route, the way the rows tests assert it
        with pytest.raises(slam.SlamHipError, match="descriptor rows are not enabled"):
            run.km.descriptor_rows(0)
    fn(run)
    assert seen["steps"] >= 3 and run.n_pos >= 5
    if name == "no_rows":
        with pytest.raises(slam.SlamHipError, match="descriptor rows are not enabled"):
            run.km.descriptor_rows(0)


def test_counts_none_enqueues_and_a_download_shows_the_same_state(dev):
    run, fn = dev("plain", want_counts=False)
    run.on_step = lambda step: run.check()
    fn(run)
    assert run.n_pos >= 5


def test_the_set_seam_agrees_where_observer_pixel_and_pose_coincide(dev, slam):
    """Sequence 1: the first observer is key-frame 0, the slot's frozen first observation is the slab's pixel, no pose has been refined.
    ks.triangulate_temporal on a copy of the lists gives the same is_3d set, positions to the same tolerance, and drops exactly the keypoints whose
    observation the map seam removes (that seam compacts them away; the map seam's list keeps them)."""
    run, fn = dev("plain")
    S = run.S
    copies = {}

    def on_step(step):
        run.check()
        if step == "add1":                                       # the lists as the map seam is about to meet them, with what a slot remembers
            for s in range(S):
                lst, kf0 = run.lists[s], run.m[s].keyframe(0)
                first = {int(i): p for i, p in zip(kf0["ids"], kf0["upx"])}
                fyx = np.array([first.get(int(i), p) for i, p in zip(lst["ids"], lst["yx"])])
                fk = np.array([0 if int(i) in first else 1 for i in lst["ids"]], dtype=np.int32)
                copies[s] = (lst["ids"].copy(), lst["yx"].copy(), fyx, fk)
    run.on_step = on_step
    fn(run)
    ks2 = slam.KeypointSet(S, run.cap)
    try:
        for s, (ids, yx, fyx, fk) in copies.items():
            ks2.upload(s, yx, np.zeros(len(ids), dtype=bool), np.zeros((len(ids), 3)), ids)
            ks2.upload_keyframe(s, fyx, np.ones(len(ids), dtype=bool))
            ks2.upload_first(s, fyx, fk, kf_count=2)
        kf_cw = np.stack([np.stack([ts.pose(k, s) for k in range(2)]) for s in range(S)])
        Twc = np.stack([np.linalg.inv(ts.pose(1, s)) for s in range(S)])
        ks2.triangulate_temporal(slam.stream_params(S, cam=ts.CAM, dist=np.zeros((S, 4))), kf_cw, Twc, np.full(S, 1, dtype=np.int32),
                                 max_error=ts.MAX_ERROR, min_depth=ts.MIN_DEPTH, min_parallax=ts.MIN_PARALLAX)
        n = 0
        for s in range(S):
            got, mine = ks2.download(s), run.ks.download(s)
            removed = sorted(c["id"] for c in run.last[s]["cand"] if c["code"] == nt.REMOVED)
            assert removed and sorted(set(int(i) for i in copies[s][0]) - set(int(i) for i in got["ids"])) == removed, s
            keep = ~np.isin(mine["ids"], removed)
            assert np.array_equal(mine["ids"][keep], got["ids"]) and np.array_equal(mine["is_3d"][keep], got["is_3d"]), s
            m3 = got["is_3d"].astype(bool)
            assert np.allclose(got["xyz"][m3], mine["xyz"][keep][m3], rtol=1e-9, atol=1e-9), s
            n += int(m3.sum())
        assert n >= 10
    finally:
        ks2.close()
