"""GPU: the key-frame map on a tracked run -- kitti05_1000 with S = 4 through benchlib.lockstep's pose loop, tracked_ba.STREAM_CFG's thresholds,
mismatch = 0 on both sides.  At every key-frame the diag callback adds the key-frame to the device map (slam_kfmap_add_keyframe, from the lists
in HBM) and to a tracked_ba.Record (from a download of the same lists), gathers both and compares them, solves the DEVICE windows with one
slam_local_ba_batch and applies that one solution to both -- on the device with the live lists following (ks given).  The refined positions
must be in the next download of the lists, the removed ids absent, and after every key-frame (the last one: the end state) the record's snapshot
equals the device read-backs.

PERIODS: run_tracked runs 2 + PERIODS key-frame periods, i.e. that many key-frames; the first key-frame of a stream has no window (its one pose
is constant), every later one has (the host model, tracked_ba.gather on this run, finds nb_3d >= min_cov_score for all four streams from
key-frame 1 on: about 1 000 keypoints, most of them stereo-triangulated, against thresholds of 25 .. 700).  Three solved windows per stream
therefore need four key-frames: PERIODS = 2, the smallest number; the test asserts the count.
Bars as in tests/test_gpu_kfmap.py: ids, flags, sets and copies array_equal; angles of a key-frame's theta within 1e-12, translation exact."""
import numpy as np
import pytest

import tracked_ba as tb

pytestmark = pytest.mark.gpu
S, PERIODS, R, MCAP = 4, 2, 16, 16384
ANGLE_TOL = 1e-12


def _theta_same(a, b, exact):
    return np.array_equal(a[3:], b[3:]) and (np.array_equal(a[:3], b[:3]) if exact else bool(np.all(np.abs(a[:3] - b[:3]) <= ANGLE_TOL)))


def test_tracked_run_device_map_equals_the_record(slam, syn):
    import torch
    from benchlib.lockstep import make_workload, run_lockstep_kpset
    wl = make_workload(slam, syn, "kitti05_1000", seed=0, streams=S)
    camt = wl["camt"]
    minc = np.array([c for c, _ in tb.STREAM_CFG], dtype=np.int32)
    recs = [tb.Record(camt, min_cov_score=int(c), mismatch=0.0) for c in minc]
    st = dict(km=None, solved=np.zeros(S, int), misses=[], written=set(), max_id=-1, n_refined=0, n_removed=0, checked=-1)

    def check_state(km):
        """snapshot of every record == the device read-backs (called after every key-frame's update: the last call sees the end state)"""
        for s, rec in enumerate(recs):
            th, x, ob, gone = tb.snapshot(rec)
            assert len(th) <= R
            for kfid, t in th.items():
                d = km.download_keyframe(s, kfid)
                assert d is not None and _theta_same(d["theta"], t, (s, kfid) in st["written"]), (s, kfid)
                px = {int(i): (float(p[0]), float(p[1])) for i, p, l in zip(d["ids"], d["upx"], d["live"]) if l}
                assert px == rec.kfs[kfid].px, (s, kfid)
            d = km.download_points(s)
            assert list(d["ids"]) == sorted(x), s
            for j, kp in enumerate(d["ids"]):
                kp = int(kp)
                assert np.array_equal(d["xyz"][j], x[kp]) and d["observers"][j] == ob[kp], (s, kp)
                mp = rec.mps[kp]
                assert (d["is_3d"][j], d["observed"][j], d["ba"][j], d["gone"][j]) == (mp.is_3d, mp.observed, mp.ba, kp in rec.gone), (s, kp)

    def diag(i, kf, pst, ks, ctx, off_now):
        if not kf:
            return
        if st["km"] is None:
            st["km"] = slam.KeyframeMap(S, ks.cap, R=R, mcap=MCAP, ctx=ctx)
        km, kfid, miss = st["km"], pst["n_kf"] - 1, st["misses"]
        lists = [ks.download(s, ctx=ctx) for s in range(S)]
        km.add_keyframe(ks, slam.stream_params(S, Tcw=pst["Tcw"], cam=camt), ctx=ctx)
        for s in range(S):
            tb.add_keyframe(recs[s], kfid, pst["Tcw"][s], lists[s])
            st["max_id"] = max(st["max_id"], int(lists[s]["ids"].max(initial=-1)))
        wins, status = km.gather(minc, ctx=ctx)
        wr = [tb.gather(r) for r in recs]
        want = [0 if w is not None and len(w["poses_ids"]) else 1 for w in wr]
        if list(status) != want:
            miss.append(f"kf {kfid}: status {list(status)} vs the record's {want}"); return
        for w in wins:
            r, c, tag = wr[w.stream], w.cache, f"kf {kfid} stream {w.stream}"
            P = len(r["poses_remap"])
            same = all(np.array_equal(a, b) for a, b in ((c.theta_const, r["theta_const"]), (c.pixels, r["pixels"]), (c.poses_ids, r["poses_ids"]), (c.points_ids, r["points_ids"]),
                                                         (w.poses_remap, r["poses_remap"]), (w.points_remap, r["points_remap"]), (w.obs_kf, r["obs_kf"]), (w.obs_kp, r["obs_kp"]),
                                                         (w.obs_in_covmap, r["obs_in_covmap"])))
            same = same and len(c.theta) == len(r["theta"]) and np.array_equal(c.theta[6 * P:], r["theta"][6 * P:])
            same = same and all(_theta_same(c.theta[6 * p:6 * p + 6], r["theta"][6 * p:6 * p + 6], (w.stream, int(w.poses_remap[p])) in st["written"]) for p in range(P))
            if not same:
                miss.append(f"{tag}: the gathered window differs from the record's")
        if miss or not wins:
            return
        slam.bundle_adjustment_batch_([w.cache for w in wins], [camt] * len(wins))
        km.update(wins, ks=ks, ctx=ctx)
        for w in wins:
            s, rec = w.stream, recs[w.stream]
            gone_before = set(rec.gone)
            tb.update(rec, wr[s], w.cache.theta, w.cache.outliers)
            st["solved"][s] += 1
            st["written"] |= {(s, int(k)) for k in w.poses_remap}
            after = ks.download(s, ctx=ctx)
            left = set(int(v) for v in after["ids"])
            removed = (rec.gone - gone_before) | {int(k) for k in w.points_remap if int(k) not in rec.mps}
            if removed & left:
                miss.append(f"kf {kfid} stream {s}: removed ids still in the list: {sorted(removed & left)[:8]}")
            st["n_removed"] += len(removed & set(int(v) for v in lists[s]["ids"]))
            if left != set(int(v) for v in lists[s]["ids"]) - rec.gone:
                miss.append(f"kf {kfid} stream {s}: the list lost or kept the wrong ids")
            kept = {int(k) for k in w.points_remap if int(k) in rec.mps}
            for j, (kp, t3) in enumerate(zip(after["ids"], after["is_3d"])):
                kp = int(kp)
                if t3 and kp in kept:
                    st["n_refined"] += 1
                    if not np.array_equal(after["xyz"][j], rec.mps[kp].xyz):
                        miss.append(f"kf {kfid} stream {s}: keypoint {kp} does not carry the refined position"); break
            before = {int(k): x for k, x, t3 in zip(lists[s]["ids"], lists[s]["xyz"], lists[s]["is_3d"])}
            for j, kp in enumerate(after["ids"]):                # nothing else in the list changes
                if int(kp) not in kept and not np.array_equal(after["xyz"][j], before[int(kp)]):
                    miss.append(f"kf {kfid} stream {s}: keypoint {int(kp)} outside the window changed"); break
        try:
            check_state(km)
            st["checked"] = kfid
        except AssertionError as e:
            miss.append(f"kf {kfid}: the device read-backs differ from the record's snapshot: {e}")

    run_lockstep_kpset(slam, torch, 0, wl, PERIODS, 2, 1, None, torch.device("cuda", 0), "host_u8", pose=True, diag=diag)
    km = st["km"]
    assert km is not None and not st["misses"], "\n".join(st["misses"][:30])
    print(f"KFMAP TRACKED: solved windows per stream {st['solved'].tolist()}, refined keypoints checked {st['n_refined']}, ids removed from the lists {st['n_removed']}, max id {st['max_id']}")
    assert (st["solved"] >= 3).all() and st["max_id"] < MCAP and st["n_refined"] > 0
    assert st["checked"] == 2 + PERIODS - 1                     # the read-backs were compared after the last key-frame: the end state
    km.close()
