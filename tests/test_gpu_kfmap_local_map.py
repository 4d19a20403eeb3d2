"""GPU: slam_kfmap_local_map_match (csrc/kfmap_lmm.inc) -- the local map staged and matched in HBM from the key-frame map -- against the model
(tests/np_kfmap_local_map.py) on the scripted scenes of tests/kfmap_lmm_scripts.py: S = 3 (stream 1 not selected at the last key-frame), cap 64 with
about 40 keypoints per list, R = 4 (slots are reused, covisible slabs forgotten mid-sequence), mcap = 128 (ids wrap, an entry changes owner with its
descriptor), a 70 x 105 image with cell 35 (a 2 x 3 grid), 8 key-frames; tests/test_kfmap_local_map_host.py shows that the scenes reach these edges,
have margin >= 1e-9 and produce pairs.  Bars: ids, orders, pairs, distances and proj_yx are array_equal (a key-frame's angles are computed on the
device; add() -- tests/kfmap_device.py, the driver this file shares with the other map tests -- holds them to 1e-12 once and hands the device's
bits to the model, so both sides form Tcw from the same theta; decisions are protected by the margin rule besides).  Every test fails without the
slam_kfmap_* entry points."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_device as kd  # noqa: E402
import kfmap_lmm_scripts as ls  # noqa: E402
import np_kfmap_filter as npf  # noqa: E402

pytestmark = pytest.mark.gpu
S = ls.S
DCAP = kd.DCAP


class Pair(kd.DeviceSide, ls.ModelRun):
    """the device map with its keypoint set beside the models, driven by the same scripted key-frames and descriptors"""
    match = ls.ModelRun.match                                      # the model's alone: these tests call device_match() and compare themselves

    def __init__(self, slam):
        super().__init__(slam, *ls.scenes())

    def snapshot(self):
        return self.device_bytes(range(S), staged=False)

    def run_to(self, n_kf, last_mask=None):
        """the shared sequence up to (and including) key-frame n_kf - 1, without its match"""
        for k in range(n_kf):
            self.add(last_mask if k == n_kf - 1 else None)
            if k < n_kf - 1 and k in ls.BA_AT:
                self.ba()


pair = kd.device_fixture(Pair, "pair")


def test_device_equals_model_stage_by_stage(pair):
    p = pair()
    n_pairs = [0] * S
    for k in range(ls.N_KF):
        last = k == ls.N_KF - 1
        before = p.km.debug_local_map(1) if last else None
        p.add(ls.LAST_MASK if last else None)
        got, want = p.device_match(), p.match()
        assert all(w["margin"] >= 1e-9 for w in want)
        p.check_match(got, want)
        for s in range(S):
            n_pairs[s] += len(got[1][s])
        if last:                                                   # the unselected stream: status 1, and what the call before staged for it is untouched
            assert got[0][1] == 1 and len(got[1][1]) == 0
            after = p.km.debug_local_map(1)
            assert len(before["lm_ids"]) > 0 and all(np.array_equal(before[key], after[key], equal_nan=True) for key in before)
        if k in ls.BA_AT:
            p.ba()
    assert min(n_pairs) >= 5


def test_host_array_path_on_downloads_agrees(pair):
    """the parent's only route -- downloads, assembly on the host, slam_local_map_match_batch -- gives the device-staged call's answers"""
    p = pair()
    p.run_to(6)
    status, pairs, dist = p.device_match()
    staged = [p.km.debug_local_map(s) for s in range(S)]
    made = [kd.assemble(p, s) for s in range(S)]
    assert [m is not None for m in made] == [st == 0 for st in status] and sum(m is not None for m in made) >= 2
    res = p.slam.local_map_matching_batch([m[0] for m in made if m is not None])
    for s, r in zip([s for s in range(S) if made[s] is not None], res):
        _, lm, kp_ids = made[s]
        assert np.array_equal(staged[s]["lm_ids"], lm) and np.array_equal(staged[s]["kp_ids"], kp_ids)
        assert np.array_equal(r["best_kp"], staged[s]["best_kp"]) and np.array_equal(r["best_dist"], staged[s]["best_dist"])
        took = np.flatnonzero(r["match"] >= 0)
        assert np.array_equal(pairs[s], np.array([(kp_ids[j], lm[r["match"][j]]) for j in took], dtype=np.int64).reshape(-1, 2))
        assert np.array_equal(dist[s], r["best_dist"][r["match"][took]]) and len(took) >= 1


def test_after_a_filter_and_after_an_update_the_removed_take_no_part(pair):
    p = pair()
    p.run_to(6)
    # a filter that removes, per stream, the covisible key-frame with the fewest 3-D points (np_kfmap_filter's rule `n_total < min_cov_score / 2`)
    minc = []
    for s in range(S):
        log = npf.filter_map(copy.deepcopy(p.m[s]), 0.999999, 0, first_kfid=0)
        minc.append(2 * (min(t for _, _, t, _ in log) + 1) if log else 0)
    removed = p.km.filter(0.999999, np.array(minc, dtype=np.int32), first_kfid=0)
    logs = [npf.filter_map(p.m[s], 0.999999, minc[s], first_kfid=0) for s in range(S)]
    assert [sorted(k for k, ex, _, _ in log if ex in ("few", "ratio")) for log in logs] == removed and sum(len(r) for r in removed) >= 2
    got, want = p.device_match(), p.match()
    p.check_match(got, want)
    for s in range(S):
        cur, d = p.nkf[s] - 1, p.km.debug_local_map(s)
        assert all(p.km.download_keyframe(s, k) is None for k in removed[s])
        gone_only = set()                                          # points seen by removed key-frames alone (besides none): no candidates any more
        for k in removed[s]:
            f = p.frames[s][k]
            gone_only |= {int(i) for i in f["ids"]} - {int(i) for kk in range(max(cur - ls.R + 1, 0), cur + 1) if kk not in removed[s] for i in p.frames[s][kk]["ids"]}
        assert not gone_only & set(int(i) for i in d["lm_ids"])
    # an update that removes points (the hashed outlier pattern flags every observation of about one point in thirteen)
    before = [set(int(i) for i in p.km.download_points(s)["ids"]) for s in range(S)]
    sol = p.ba()
    assert len(sol) >= 2
    got, want = p.device_match(), p.match()
    p.check_match(got, want)
    n_removed = 0
    for s in range(S):
        now = set(int(i) for i in p.km.download_points(s)["ids"])
        d = p.km.debug_local_map(s)
        n_removed += len(before[s] - now)
        assert not (before[s] - now) & (set(int(i) for i in d["lm_ids"]) | set(int(i) for i in d["kp_ids"]))
        assert not (before[s] - now) & set(int(i) for i in got[1][s].reshape(-1))
    assert n_removed >= 3


def test_a_local_map_that_does_not_fit_is_status_2_and_leaves_the_others_alone(pair):
    p = pair()
    p.run_to(6)
    full, want = p.device_match(), p.match()
    p.check_match(full, want)
    sizes = [len(w["lm_ids"]) for w in want]
    big = int(np.argmax(sizes))
    assert sizes[big] > max(sizes[s] for s in range(S) if s != big) >= 1
    got = p.device_match(max_local=sizes[big] - 1)
    want2 = p.match(max_local=sizes[big] - 1)
    assert [w["status"] for w in want2] == [2 if s == big else want[s]["status"] for s in range(S)]
    p.check_match(got, want2, staged=False)
    assert len(got[1][big]) == 0 and len(p.km.debug_local_map(big)["lm_ids"]) == 0
    for s in range(S):
        if s != big:
            assert np.array_equal(got[1][s], full[1][s]) and np.array_equal(got[2][s], full[2][s])
    exact = p.device_match(max_local=sizes[big])                    # exactly as large as the bound: fits
    p.check_match(exact, want)


def test_the_call_has_no_side_effects(pair):
    p = pair()
    p.run_to(6)
    before = p.snapshot()
    a = p.device_match()
    da = [p.km.debug_local_map(s) for s in range(S)]
    b = p.device_match()
    db = [p.km.debug_local_map(s) for s in range(S)]
    assert a[0].tobytes() == b[0].tobytes()
    for s in range(S):
        assert a[1][s].tobytes() == b[1][s].tobytes() and a[2][s].tobytes() == b[2][s].tobytes()
        assert all(da[s][key].tobytes() == db[s][key].tobytes() for key in da[s])
    assert p.snapshot() == before
    assert sum(len(x) for x in a[1]) >= 3


def test_argument_errors_launch_nothing(pair, slam):
    p = pair()
    p.run_to(5)
    good = p.device_match()
    staged = [p.km.debug_local_map(s) for s in range(S)]
    cam = np.tile(np.array(ls.CAM10), (S, 1))
    cam[1, 6] = 1e-4                                               # p1 of one stream
    with pytest.raises(slam.SlamHipError, match="distortion"):
        p.km.local_map_match(cam, ls.CELL, 2.0, 0.35)
    for s in range(S):                                             # nothing was staged over the last call's regions
        d = p.km.debug_local_map(s)
        assert all(np.array_equal(d[key], staged[s][key], equal_nan=True) for key in d)
    plain = slam.KeyframeMap(S, ls.CAP, R=ls.R, mcap=ls.MCAP)
    try:
        with pytest.raises(slam.SlamHipError, match="not enabled"):
            plain.local_map_match(ls.CAM10, ls.CELL, 2.0, 0.35)
        with pytest.raises(slam.SlamHipError, match="not enabled"):
            plain.add_descriptors(1, 1, DCAP)
        with pytest.raises(slam.SlamHipError, match="256"):
            plain.enable_descriptors(128)
    finally:
        plain.close()
    again = p.device_match()
    assert all(np.array_equal(x, y) for x, y in zip(good[1], again[1]))
