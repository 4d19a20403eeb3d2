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
import kfmap_device as kd  # noqa: E402
import kfmap_tri_scripts as ts  # noqa: E402
import np_kfmap_tri as nt  # noqa: E402

pytestmark = pytest.mark.gpu
DCAP = 320


class Dev(kd.DeviceSide, ts.TriRun):
    """the device map with its keypoint set beside the models, driven through the same steps"""
    dcap = DCAP

    def __init__(self, slam, want_counts=True, **kw):
        rows = kw.get("rows", 0)
        super().__init__(slam, descriptors=bool(rows), descriptor_rows=rows or None, **kw)
        self.want_counts, self.n_pos = want_counts, 0

    @property
    def kset(self):
        return self.ks if self.with_list else None

    def took_parts(self, took):
        """the lists as they are; the rows of the ids born at this key-frame (consecutive: one block per stream)"""
        if not self.rows:
            return took, None
        desc = {}
        for s, f in took.items():
            born = self.tracks[s][self.nkf[s] - 1][1]
            new = [int(i) for i in f["ids"] if int(i) >= born]
            if new:
                desc[s] = (new[0], self.desc_rows(s, new))
        return took, desc

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
        self.device_gather(want)                                 # the gather searched the slabs the triangulation wrote: the window is the model's
        return want

    def update(self, wins, sols):
        super().update(wins, sols)
        self.device_update(sols)


dev = kd.device_fixture(Dev, "dev", through=ts.make)


@pytest.mark.parametrize("name", sorted(ts.SEQUENCES))
def test_device_equals_model_after_every_step(dev, slam, name):
    run, fn = dev(name)
    seen = dict(steps=0, before=None)

    def on_step(step):
        run.check()
        seen["steps"] += 1
        if name == "selection" and step == "add2":                # 7: the unselected stream's bytes, before the call
            seen["before"] = run.device_bytes([1], staged=False)
        if name == "selection" and step == "tri2":
            assert run.device_bytes([1], staged=False) == seen["before"] and run.last[1] is None
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
