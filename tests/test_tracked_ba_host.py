"""CPU: the tracked-window gatherer of tests/tracked_ba.py (_get_ba_parameters / _update_ba_parameters!, src/estimator.jl:143-306) on a
hand-built map whose window is worked out by hand, and the frozen tracked windows of tests/golden/tracked_ba_v1.npz against the oracle
and the independent numpy Jacobian of tests/np_ba.py."""
import os

import numpy as np
import pytest

import tracked_ba as tb

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "tracked_ba_v1.npz")


def _map():
    """Eight key-frames, min_cov_score 3.  Map points (kpid: observers):
    10: 0 5 6   11: 0 6   12: 0 6 7   13: 3 5 6   14: 5 6   15: 6 (seen by the current frame)   21: 6 (2-D)
    16: 2 5     17: 5 (not seen by the current frame: bad)   18: 0 1   19: 3 4   20: 7
    Key-frame 6 is the BA's; key-frame 7 (the mapper ran ahead) is newer.  Scores of key-frame 6: 0 -> 3, 3 -> 1, 5 -> 3, 7 -> 1, itself 6;
    key-frames 1, 2 and 4 share no point with it, so its covisibility map is {7, 6, 5, 3, 0}."""
    rec = tb.Record((700.0, 710.0, 600.0, 180.0), min_cov_score=3)
    obs = {10: (0, 5, 6), 11: (0, 6), 12: (0, 6, 7), 13: (3, 5, 6), 14: (5, 6), 15: (6,), 21: (6,),
           16: (2, 5), 17: (5,), 18: (0, 1), 19: (3, 4), 20: (7,)}
    for k in range(8):
        rec.kfs[k] = tb.KeyFrame([0.01 * k, -0.02 * k, 0.003 * k, 0.1 * k, -0.05 * k, 0.7 * k], {})
    for kp, ob in obs.items():
        rec.mps[kp] = tb.MapPoint([kp * 0.1, -kp * 0.05, 10.0 + kp], ob, kp in (10, 11, 12, 13, 14, 15, 21), kp != 21)
        for k in ob:
            rec.kfs[k].px[kp] = (100.0 + kp, 200.0 + 10 * k)
    rec.cur = 6
    return rec


# (kpid, kfid) of every observation in the order _get_ba_parameters emits them
_OBS = [(10, 0), (10, 5), (10, 6), (11, 0), (11, 6), (12, 0), (12, 6), (13, 3), (13, 5), (13, 6), (14, 5), (14, 6), (15, 6),
        (16, 2), (16, 5), (19, 3), (19, 4), (18, 0), (18, 1)]


def test_gather_on_a_hand_built_map():
    rec = _map()
    w = tb.gather(rec, 6)
    assert list(w["covmap"].items()) == [(7, 1), (6, 6), (5, 3), (3, 1), (0, 3)]        # 5 newest, newest first
    # pose order = first encounter: 0 (point 10), 5, 6, 3 (point 13), 2 (point 16 of key-frame 5), 4 (point 19 of key-frame 3), 1 (point 18 of key-frame 0)
    assert w["poses_remap"].tolist() == [0, 5, 6, 3, 2, 4, 1]
    # constant: 0 (kfid 0, though its score 3 is not low), 3 (score 1 < 3), 2 / 4 / 1 (observers outside the covisibility map); 7 never enters (newer)
    assert w["theta_const"].tolist() == [1, 0, 0, 1, 1, 1, 1]
    # points: key-frame 6's 3-D points, then key-frame 5's new ones (17 is bad), then 3's, then 0's; 21 is 2-D, 20 only in the newer key-frame
    assert w["points_remap"].tolist() == [10, 11, 12, 13, 14, 15, 16, 19, 18]
    assert w["bad"] == {17} and not rec.mps[17].is_3d
    assert list(zip(w["obs_kp"].tolist(), w["obs_kf"].tolist())) == _OBS
    pose_of = {k: i + 1 for i, k in enumerate(w["poses_remap"].tolist())}
    pt_of = {k: i + 1 for i, k in enumerate(w["points_remap"].tolist())}
    assert w["poses_ids"].tolist() == [pose_of[kf] for _, kf in _OBS]
    assert w["points_ids"].tolist() == [pt_of[kp] for kp, _ in _OBS]
    assert w["obs_in_covmap"].tolist() == [kf in (7, 6, 5, 3, 0) for _, kf in _OBS]
    assert np.array_equal(w["pixels"], np.array([(100.0 + kp, 200.0 + 10 * kf) for kp, kf in _OBS]))
    P = 7
    for i, k in enumerate(w["poses_remap"]):
        assert np.array_equal(w["theta"][6 * i:6 * i + 6], rec.kfs[int(k)].theta)
    for i, kp in enumerate(w["points_remap"]):
        assert np.array_equal(w["theta"][6 * P + 3 * i:6 * P + 3 * i + 3], rec.mps[int(kp)].xyz)
    st = tb.structure(w)
    # 15: one observer, a free pose; 19 / 18: constant observers only (16 has the free 5 as well); four constant poses besides key-frame 0
    assert (st["P"], st["free"], st["M"], st["O"], st["single_free"], st["const_only"], st["const_not0"]) == (7, 2, 9, 19, 1, 2, 4)
    # too few 3-D keypoints at the key-frame (1 < 3): no BA
    assert tb.gather(rec, 1) is None


def test_update_on_a_hand_made_cache():
    rec = _map()
    w = tb.gather(rec, 6)
    P, M = 7, 9
    theta = w["theta"] + 0.25 + np.arange(len(w["theta"])) * 1e-3
    outl = np.zeros(len(_OBS), dtype=bool)
    for kp, kf in ((15, 6), (16, 2), (11, 0), (14, 5), (19, 3)):
        outl[_OBS.index((kp, kf))] = True
    tb.update(rec, w, theta, outl)
    for i, k in enumerate(w["poses_remap"]):
        assert np.array_equal(rec.kfs[int(k)].theta, theta[6 * i:6 * i + 6])
    # 15: its one observation was the current key-frame's -> dropped from the key-frame and the current frame, then bad -> removed
    # 19: its observation by key-frame 3 (in the map) dropped; one observer left and not seen now -> removed (key-frame 4 loses it too)
    assert 15 not in rec.mps and 19 not in rec.mps and rec.gone == {15}
    assert 15 not in rec.kfs[6].px and 19 not in rec.kfs[3].px and 19 not in rec.kfs[4].px
    # 16: the outlier observer 2 lies outside the map -> kept; 11 / 14: observations by 0 / 5 dropped, still seen now -> kept
    assert rec.mps[16].obs == {2, 5} and 16 in rec.kfs[2].px
    assert rec.mps[11].obs == {6} and 11 not in rec.kfs[0].px and rec.mps[14].obs == {6} and 14 not in rec.kfs[5].px
    # 17 was demoted to 2-D by the gather: is_bad! no longer holds for it and it stays
    assert 17 in rec.mps and not rec.mps[17].is_3d
    for i, kp in enumerate(w["points_remap"].tolist()):
        if kp in rec.mps:
            assert np.array_equal(rec.mps[kp].xyz, theta[6 * P + 3 * i:6 * P + 3 * i + 3]) and rec.mps[kp].ba, kp
    assert sorted(rec.mps) == [10, 11, 12, 13, 14, 16, 17, 18, 20, 21]
    # a key-frame recorded afterwards skips the ids the current frame lost and does not move a point a BA has placed
    lst = dict(ids=np.array([10, 15, 22]), yx=np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]), is_3d=np.array([True, True, True]),
               xyz=np.array([[9.0, 9.0, 9.0], [8.0, 8.0, 8.0], [7.0, 7.0, 7.0]]))
    x10 = rec.mps[10].xyz.copy()
    tb.add_keyframe(rec, 8, np.eye(4), lst)
    assert sorted(rec.kfs[8].px) == [10, 22] and 15 not in rec.mps
    assert np.array_equal(rec.mps[10].xyz, x10) and rec.mps[10].obs == {0, 5, 6, 8}
    assert rec.mps[22].obs == {8} and np.array_equal(rec.mps[22].xyz, [7.0, 7.0, 7.0])
    assert not rec.mps[11].observed and rec.mps[10].observed


def _windows():
    if not os.path.exists(GOLDEN):
        pytest.fail(f"{GOLDEN} is missing: run tests/golden/make_golden_tracked_ba.py on a GPU machine")
    z = np.load(GOLDEN)
    n = int(z["n"])
    out = []
    for k in range(n):
        g = lambda key: z[f"w{k}_{key}"]
        out.append(dict(tag=str(g("tag")), cam=g("cam"), theta0=g("theta0"), theta_const=g("theta_const"), pixels=g("pixels"),
                        poses_ids=g("poses_ids").astype(np.int64), points_ids=g("points_ids").astype(np.int64),
                        theta=g("theta"), outliers=g("outliers").astype(bool), stats=g("stats")))
    return out


def test_golden_tracked_windows_cover_stereo_and_mono():
    ws = _windows()
    tags = [w["tag"] for w in ws]
    assert any(t.startswith("stereo") for t in tags) and any(t.startswith("mono") for t in tags), tags
    assert os.path.getsize(GOLDEN) <= 512 * 1024
    st = [tb.structure(dict(w, theta=w["theta0"], poses_remap=np.arange(len(w["theta_const"])))) for w in ws]
    assert sum(s["single_free"] for s in st) > 0 and sum(s["const_only"] for s in st) > 0, st
    assert sum(s["const_not0"] for s in st) > 0 and sum(int(w["outliers"].sum()) for w in ws) > 0, st


def test_oracle_reproduces_the_golden_tracked_windows(orc):
    for w in _windows():
        th, ol, st = orc.bundle_adjustment(w["cam"], w["theta0"], w["theta_const"], w["pixels"], w["poses_ids"], w["points_ids"], 5, 10, 5.0, solver=1)
        assert np.array_equal(ol, w["outliers"]), w["tag"]
        assert abs(st["ssr_final"] - w["stats"][0]) <= 1e-10 * w["stats"][0], w["tag"]
        assert np.abs(th - w["theta"]).max() <= 1e-9 * max(1.0, np.abs(w["theta"]).max()), w["tag"]


def _grad(w, theta):
    """J^T r over the inlier observations, free poses and all points (np_ba's complex-step Jacobian)"""
    import np_ba
    P = len(w["theta_const"])
    poses, pts = theta[:6 * P].reshape(P, 6), theta[6 * P:].reshape(-1, 3)
    keep = ~w["outliers"]
    pi, li, px = w["poses_ids"][keep] - 1, w["points_ids"][keep] - 1, w["pixels"][keep]
    r = np_ba.residuals(w["cam"], poses, pts, px, pi, li)
    Jp, Jl = np_ba.jacobians(w["cam"], poses, pts, px, pi, li)
    gp = np.zeros((P, 6)); gl = np.zeros_like(pts)
    np.add.at(gp, pi, np.einsum("oki,ok->oi", Jp, r))
    np.add.at(gl, li, np.einsum("oki,ok->oi", Jl, r))
    gp[w["theta_const"].astype(bool)] = 0.0
    return np.sqrt((gp ** 2).sum() + (gl ** 2).sum())


def test_golden_tracked_solutions_are_a_real_descent():
    """at the solution the inlier gradient is at least 1e3 below its value at theta0, by a Jacobian formed independently of the oracle's"""
    for w in _windows():
        g0, g1 = _grad(w, w["theta0"]), _grad(w, w["theta"])
        assert g1 * 1e3 <= g0, (w["tag"], g0, g1)
