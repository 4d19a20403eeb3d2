"""GPU: slam_kfmap_local_map_match (csrc/kfmap_lmm.inc) -- the local map staged and matched in HBM from the key-frame map -- against the model
(tests/np_kfmap_local_map.py) on the scripted scenes of tests/kfmap_lmm_scripts.py: S = 3 (stream 1 not selected at the last key-frame), cap 64 with
about 40 keypoints per list, R = 4 (slots are reused, covisible slabs forgotten mid-sequence), mcap = 128 (ids wrap, an entry changes owner with its
descriptor), a 70 x 105 image with cell 35 (a 2 x 3 grid), 8 key-frames; tests/test_kfmap_local_map_host.py shows that the scenes reach these edges,
have margin >= 1e-9 and produce pairs.  Bars: ids, orders, pairs and distances are array_equal; proj_yx within 1e-9 px (the device forms Tcw from
theta by angles_to_pose, the model by the same formula in numpy: the sines and cosines may differ in the last place; decisions are protected by the
margin rule).  Every test fails without the slam_kfmap_* entry points."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_lmm_scripts as ls  # noqa: E402
import kfmap_scripts as scr  # noqa: E402
import np_kfmap_filter as npf  # noqa: E402
import np_kfmap_local_map as nl  # noqa: E402

pytestmark = pytest.mark.gpu
S = ls.S
PX_TOL = 1e-9
DCAP = 64


class Pair(ls.ModelRun):
    """the device map with its keypoint set beside the models, driven by the same scripted key-frames and descriptors"""

    def __init__(self, slam):
        import torch
        self.torch, self.slam = torch, slam
        frames, descs = ls.scenes()
        super().__init__(frames, descs)
        self.ks = slam.KeypointSet(S, ls.CAP)
        self.km = slam.KeyframeMap(S, ls.CAP, R=ls.R, mcap=ls.MCAP)
        self.km.enable_descriptors()
        self.Tcw = np.tile(np.eye(4), (S, 1, 1))
        self.rows = [dict() for _ in range(S)]                     # id -> row, as the script handed them out (the cross-check's descriptors)

    def close(self):
        self.km.close(); self.ks.close()

    def add(self, mask=None):
        took = super().add(mask)
        desc = np.full((S, DCAP, 4), 0x5555555555555555, dtype=np.uint64)       # an unselected stream offers rows too: they must not be taken
        info = np.zeros((S, 2), dtype=np.int64)
        for s in range(S):
            info[s] = (10 ** 6, 3)
        for s, (f, d) in took.items():
            self.ks.upload(s, f["yx"], f["is_3d"], f["xyz"], f["ids"])
            self.Tcw[s] = f["Tcw"]
            info[s] = (d[0], len(d[1])); desc[s, :len(d[1])] = d[1]
            self.rows[s].update({int(d[0]) + j: r for j, r in enumerate(d[1])})
        sp = self.slam.stream_params(S, Tcw=self.Tcw, cam=ls.CAM10[:4], dist=np.zeros((S, 4)))
        desc_dev = self.torch.from_numpy(desc.view(np.int64)).cuda(); info_dev = self.torch.from_numpy(info).cuda()
        with self.ks.selected(mask):
            self.ks.keyframe()
            self.km.add_keyframe(self.ks, sp)
            self.km.add_descriptors(desc_dev.data_ptr(), info_dev.data_ptr(), DCAP)
        self.km.ctx.synchronize()                                  # (the device arrays above live until the copies have run)
        return took

    def device_match(self, **kw):
        return self.km.local_map_match(ls.CAM10, ls.CELL, ls.PARAMS.max_projection_distance, ls.PARAMS.max_descriptor_distance, **kw)

    def ba(self):
        wins, status = self.km.gather(np.full(S, self.m[0].min_cov_score, dtype=np.int32))
        sol = super().ba()
        assert [w.stream for w in wins] == sorted(sol)
        self.km.update(wins, [sol[w.stream][1] for w in wins], [sol[w.stream][2] for w in wins])
        return sol

    def check(self, got, want, staged=True):
        status, pairs, dist = got
        assert list(status) == [w["status"] for w in want]
        for s in range(S):
            assert pairs[s].dtype == np.int64 and np.array_equal(pairs[s], want[s]["pairs"]), s
            assert np.array_equal(dist[s], want[s]["dist"]), s
            if not staged or not self.sel[s]:
                continue
            d, w = self.km.debug_local_map(s), want[s]
            assert np.array_equal(d["lm_ids"], w["lm_ids"]) and np.array_equal(d["kp_ids"], w["kp_ids"]), s
            assert np.array_equal(d["best_kp"], w["best_kp"]) and np.array_equal(d["best_dist"], w["best_dist"]), s
            assert np.array_equal(np.isnan(d["proj_yx"]), np.isnan(w["proj_yx"])), s
            ok = ~np.isnan(w["proj_yx"])
            assert np.all(np.abs(d["proj_yx"][ok] - w["proj_yx"][ok]) <= PX_TOL), s

    def snapshot(self):
        out = []
        for s in range(S):
            d = [self.km.download_points(s)] + [self.km.download_keyframe(s, k) for k in range(self.nkf[s] + 1)]
            out.append(repr([(sorted((k, np.asarray(v).tobytes() if not isinstance(v, list) else repr(v)) for k, v in x.items()) if x is not None else None) for x in d]))
        return out

    def run_to(self, n_kf, last_mask=None):
        """the shared sequence up to (and including) key-frame n_kf - 1, without its match"""
        for k in range(n_kf):
            self.add(last_mask if k == n_kf - 1 else None)
            if k < n_kf - 1 and k in ls.BA_AT:
                self.ba()


@pytest.fixture()
def pair(slam):
    made = []

    def make():
        made.append(Pair(slam))
        return made[-1]
    yield make
    for p in made:
        p.close()


def test_device_equals_model_stage_by_stage(pair):
    p = pair()
    n_pairs = [0] * S
    for k in range(ls.N_KF):
        last = k == ls.N_KF - 1
        before = p.km.debug_local_map(1) if last else None
        p.add(ls.LAST_MASK if last else None)
        got, want = p.device_match(), p.match()
        assert all(w["margin"] >= 1e-9 for w in want)
        p.check(got, want)
        for s in range(S):
            n_pairs[s] += len(got[1][s])
        if last:                                                   # the unselected stream: status 1, and what the call before staged for it is untouched
            assert got[0][1] == 1 and len(got[1][1]) == 0
            after = p.km.debug_local_map(1)
            assert len(before["lm_ids"]) > 0 and all(np.array_equal(before[key], after[key], equal_nan=True) for key in before)
        if k in ls.BA_AT:
            p.ba()
    assert min(n_pairs) >= 5


def _assemble(p, s):
    """the arrays of the host-array path from DOWNLOADS of stream s's map (download_keyframe, download_points) and the script's descriptor rows, stated on
    dicts and sets -> (frame, keypoints, keyframes, local_map, params), the local-map ids, the keypoint ids; None where there is nothing to match"""
    cur = int(p.km.newest()[s])
    kfs = {k: d for k in range(max(cur - ls.R + 1, 0), cur + 1) for d in [p.km.download_keyframe(s, k)] if d is not None}
    pts = p.km.download_points(s)
    point = {int(i): j for j, i in enumerate(pts["ids"])}
    rows = p.rows[s]
    live = {k: {int(i): tuple(px) for i, px, lv in zip(d["ids"], d["upx"], d["live"]) if lv} for k, d in kfs.items()}
    if cur not in kfs:
        return None
    cov = set()
    for i in live[cur]:
        if i in point:
            cov |= {o for o in pts["observers"][point[i]] if o != cur and o in kfs}
    lm = sorted({i for o in cov for i in live[o] if i in point and pts["is_3d"][point[i]] and i in rows and cur not in pts["observers"][point[i]]})
    order = sorted(kfs)
    row = {k: j for j, k in enumerate(order)}
    kp_ids = [i for i in live[cur] if i in point and i in rows]
    if not cov or not lm or not kp_ids:
        return None
    keypoints = [{"pixel": live[cur][i], "descriptors": rows[i].reshape(1, 4),
                  "observers": [(row[o], live[o][i]) for o in pts["observers"][point[i]] if o in kfs and i in live[o]]} for i in kp_ids]
    local_map = [{"position": pts["xyz"][point[i]], "descriptors": rows[i].reshape(1, 4), "observers": [row[o] for o in pts["observers"][point[i]] if o in kfs]} for i in lm]
    nb3 = sum(1 for i in live[cur] if i in point and pts["is_3d"][point[i]])
    frame = {"Tcw": nl.tcw_of(kfs[cur]["theta"]), "cam": ls.CAM10, "cell_size": ls.CELL, "nb_3d_kpts": nb3}
    return (frame, keypoints, np.array([nl.tcw_of(kfs[k]["theta"]) for k in order]), local_map, ls.PARAMS), lm, kp_ids


def test_host_array_path_on_downloads_agrees(pair):
    """the parent's only route -- downloads, assembly on the host, slam_local_map_match_batch -- gives the device-staged call's answers"""
    p = pair()
    p.run_to(6)
    status, pairs, dist = p.device_match()
    staged = [p.km.debug_local_map(s) for s in range(S)]
    made = [_assemble(p, s) for s in range(S)]
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
    p.check(got, want)
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
    p.check(got, want)
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
    p.check(full, want)
    sizes = [len(w["lm_ids"]) for w in want]
    big = int(np.argmax(sizes))
    assert sizes[big] > max(sizes[s] for s in range(S) if s != big) >= 1
    got = p.device_match(max_local=sizes[big] - 1)
    want2 = p.match(max_local=sizes[big] - 1)
    assert [w["status"] for w in want2] == [2 if s == big else want[s]["status"] for s in range(S)]
    p.check(got, want2, staged=False)
    assert len(got[1][big]) == 0 and len(p.km.debug_local_map(big)["lm_ids"]) == 0
    for s in range(S):
        if s != big:
            assert np.array_equal(got[1][s], full[1][s]) and np.array_equal(got[2][s], full[2][s])
    exact = p.device_match(max_local=sizes[big])                    # exactly as large as the bound: fits
    p.check(exact, want)


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
