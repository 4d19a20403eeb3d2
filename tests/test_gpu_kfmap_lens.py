"""GPU: the key-frame map with raw pixels (slam_kfmap_enable_pixels, csrc/kfmap.hpp) behind a lens -- the local-map match staged from kp.pixel, the
merge that moves the raw pixels with the renamed observations -- against the model of tests/kfmap_lens_scripts.py on its scenes: the scenes of
tests/kfmap_lmm_scripts.py (S = 3, cap 64, R = 4, mcap = 128, a 70 x 105 image with cell 35, 8 key-frames, stream 1 not selected at the last, a
local-BA update behind key-frames 3 and 4) seen through dist = (-0.28, 0.07, 2e-4, 2e-5).  tests/test_kfmap_lens_host.py shows that the model pairs on
every stream with margins >= 1e-9, that the lens moves pixels by more than the projection gate, and that a match on the wrong pixels or with the
wrong camera gives other pairs.

After EVERY step the status, pairs, distances, the staged kp_ids / lm_ids / best_kp / best_dist and keyframe_pixels of every ring slot are array_equal
to the model; proj_yx within 1e-9 px (the device forms Tcw from theta by angles_to_pose and projects through the lens in its own arithmetic).  The
slabs' ids and live bytes are array_equal; their undistorted pixels are the device's undistort_px of the raw pixel and are held to 1e-9 px (the
kernel may contract multiply-adds; nothing in these sequences decides on them).  A key-frame's angles are computed on the device; add() holds them to
1e-12 once and hands the device's bits to the model, as tests/test_gpu_kfmap_merge.py does.  Every test fails without slam_kfmap_enable_pixels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_lens_scripts as lz  # noqa: E402
import kfmap_lmm_scripts as ls  # noqa: E402
import kfmap_merge_scripts as ms  # noqa: E402
import np_kfmap_local_map as nl  # noqa: E402
import np_kfmap_rows as nr  # noqa: E402

pytestmark = pytest.mark.gpu
S = ls.S
DCAP = 64
PX_TOL = 1e-9
ANGLE_TOL = 1e-12


class Dev(lz.LensRun):
    """the device map with its keypoint set beside the models, driven by the same scripted key-frames and descriptors; pixels=False: a map that
    never enables the raw pixels"""

    def __init__(self, slam, dist=lz.DIST, mode="stale", kind="plain", pixels=True):
        import torch
        self.torch, self.slam = torch, slam
        super().__init__(dist=dist, mode=mode, kind=kind)
        self.ks = slam.KeypointSet(S, ls.CAP)
        self.km = slam.KeyframeMap(S, ls.CAP, R=ls.R, mcap=ls.MCAP)
        self.km.enable_descriptors()
        if kind == "rows":
            self.km.enable_descriptor_rows(2)
        if kind == "history":
            self.km.enable_local_map_history()
        if pixels:
            self.km.enable_pixels()
            self.km.enable_pixels()                              # a second call is a no-op
        self.has_pixels = pixels
        self.Tcw = np.tile(np.eye(4), (S, 1, 1))
        self.rows = [dict() for _ in range(S)]                   # id -> row, as the script handed them out (the cross-check's descriptors)

    def close(self):
        self.km.close(); self.ks.close()

    @property
    def kset(self):
        return self.ks if self.mode == "follow" else None

    def add(self, mask=None):
        took = super().add(mask)
        desc = np.full((S, DCAP, 4), 0x5555555555555555, dtype=np.uint64)       # an unselected stream offers rows too: they must not be taken
        info = np.tile(np.array([10 ** 6, 3], dtype=np.int64), (S, 1))
        for s, (f, d) in took.items():
            self.ks.upload(s, f["yx"], f["is_3d"], f["xyz"], f["ids"])
            self.Tcw[s] = f["Tcw"]
            info[s] = (d[0], len(d[1])); desc[s, :len(d[1])] = d[1]
            self.rows[s].update({int(d[0]) + j: r for j, r in enumerate(d[1])})
        sp = self.slam.stream_params(S, Tcw=self.Tcw, cam=lz.CAM4, dist=np.tile(np.array(self.dist), (S, 1)))
        desc_dev = self.torch.from_numpy(desc.view(np.int64)).cuda(); info_dev = self.torch.from_numpy(info).cuda()
        with self.ks.selected(mask):
            self.ks.keyframe()
            self.km.add_keyframe(self.ks, sp)
            self.km.add_descriptors(desc_dev.data_ptr(), info_dev.data_ptr(), DCAP)
        self.km.ctx.synchronize()                                # (the device arrays above live until the copies have run)
        for s in took:                                           # the device's angles, checked to their bar, become the model's
            k = self.nkf[s] - 1
            th, ref = self.km.download_keyframe(s, k)["theta"], self.m[s].theta[k % ls.R]
            assert np.array_equal(th[3:], ref[3:]) and np.all(np.abs(th[:3] - ref[:3]) <= ANGLE_TOL), (s, k)
            self.m[s].theta[k % ls.R] = th
        return took

    def device_match(self, **kw):
        return self.km.local_map_match(self.cam, ls.CELL, ls.PARAMS.max_projection_distance, ls.PARAMS.max_descriptor_distance, **kw)

    def match(self, **kw):
        """the model's match, the device's checked against it: results and staged lists"""
        want = super().match(**kw)
        status, pairs, dist = self.device_match()
        assert all(w["margin"] >= 1e-9 for w in want)
        assert list(status) == [w["status"] for w in want]
        for s in range(S):
            assert pairs[s].dtype == np.int64 and np.array_equal(pairs[s], want[s]["pairs"]), s
            assert np.array_equal(dist[s], want[s]["dist"]), s
            if not self.sel[s]:
                continue
            d, w = self.km.debug_local_map(s), want[s]
            assert np.array_equal(d["lm_ids"], w["lm_ids"]) and np.array_equal(d["kp_ids"], w["kp_ids"]), s
            assert np.array_equal(d["best_kp"], w["best_kp"]) and np.array_equal(d["best_dist"], w["best_dist"]), s
            assert np.array_equal(np.isnan(d["proj_yx"]), np.isnan(w["proj_yx"])), s
            ok = ~np.isnan(w["proj_yx"])
            assert np.all(np.abs(d["proj_yx"][ok] - w["proj_yx"][ok]) <= PX_TOL), s
        return want

    def merge(self, pairs):
        """the model's merge of `pairs`, the device's of the pairs its last match left in HBM"""
        want = super().merge(pairs).copy()
        got = self.km.merge(self.kset, None)
        assert np.array_equal(got, want), (got, want)
        return want

    def ba(self):
        wins, status = self.km.gather(np.full(S, self.m[0].min_cov_score, dtype=np.int32))
        sol = super().ba()
        assert [w.stream for w in wins] == sorted(sol)
        for w in wins:                                           # the gather reads the UNDISTORTED pixels, whatever the match reads
            ref = sol[w.stream][0]
            assert np.array_equal(w.obs_kf, ref["obs_kf"]) and np.array_equal(w.obs_kp, ref["obs_kp"]) and np.array_equal(w.points_remap, ref["points_remap"])
            assert np.all(np.abs(w.cache.pixels - ref["pixels"]) <= PX_TOL)
        self.km.update(wins, [sol[w.stream][1] for w in wins], [sol[w.stream][2] for w in wins], ks=self.kset)
        return sol

    def check(self):
        """every ring slot: the raw pixels, ids and live bytes exactly, the undistorted pixels to rounding; the points; the live lists"""
        for s, m in enumerate(self.m):
            for k in range(max(m.cur - ls.R + 1, 0), m.cur + 2):
                d, w = self.km.download_keyframe(s, k), m.keyframe(k)
                px = self.km.keyframe_pixels(s, k) if self.has_pixels else None
                assert (d is None) == (w is None), (s, k)
                if w is None:
                    assert px is None
                    continue
                assert all(np.array_equal(d[key], w[key]) for key in ("theta", "ids", "live")), (s, k)
                assert d["upx"].shape == w["upx"].shape and np.all(np.abs(d["upx"] - w["upx"]) <= PX_TOL), (s, k)
                if self.has_pixels:
                    assert px.shape == (len(w["ids"]), 2) and np.array_equal(px, self.pixels(s, k)), (s, k)
            d, w = self.km.download_points(s), m.points()
            assert all(np.array_equal(d[key], w[key]) for key in ("ids", "xyz", "is_3d", "observed", "ba", "gone")) and d["observers"] == w["observers"], s
            if self.kset is not None and self.lists[s] is not None:
                d = self.ks.download(s)
                assert all(np.array_equal(d[key], self.lists[s][key]) for key in ("ids", "yx", "is_3d", "xyz")), s
            if self.kind == "rows":
                assert nr.same_rows(self.km.descriptor_rows(s), nr.descriptor_rows(m, self.D[s])), s


@pytest.fixture()
def dev(slam):
    made = []

    def make(**kw):
        made.append(Dev(slam, **kw))
        return made[-1]
    yield make
    for p in made:
        p.close()


def run_checked(p, merges):
    seen = dict(pairs=np.zeros(S, dtype=np.int64), applied=0, renamed=0)

    def on_step(kind, k, data):
        p.check()
        if kind == "match":
            seen["pairs"] += [len(r["pairs"]) for r in data]
        if kind == "merge":
            seen["applied"] += int(p.counts[:, 0].sum()); seen["renamed"] += int(p.counts[:, 2].sum())
    lz.run_sequence(p, merges=merges, on_step=on_step)
    return seen


def test_device_equals_model_after_every_step(dev):
    seen = run_checked(dev(), merges=False)
    assert list(seen["pairs"]) == [41, 30, 11]                   # the counts tests/test_kfmap_lens_host.py reports for the model


@pytest.mark.parametrize("mode", ms.MODES)
def test_raw_pixels_follow_the_merged_observations(dev, mode):
    """merge() behind every match -- with the keypoint set (the lists follow) and without: the rebuilt slabs hold every raw pixel beside its id"""
    seen = run_checked(dev(mode=mode), merges=True)
    assert min(seen["pairs"]) >= 5 and seen["applied"] >= 10 and seen["renamed"] >= seen["applied"]


@pytest.mark.parametrize("kind", ("history", "rows"))
def test_with_the_history_and_with_descriptor_rows(dev, kind):
    seen = run_checked(dev(kind=kind, mode="follow"), merges=True)
    assert min(seen["pairs"]) >= 5 and seen["applied"] >= 10


def _assemble(p, s):
    """the arrays of the host-array path from DOWNLOADS of stream s's map -- download_keyframe for ids and live bytes, keyframe_pixels for the RAW
    pixels, download_points -- and the script's descriptor rows, stated on dicts and sets -> (problem, local-map ids, keypoint ids), or None"""
    cur = int(p.km.newest()[s])
    kfs = {k: d for k in range(max(cur - ls.R + 1, 0), cur + 1) for d in [p.km.download_keyframe(s, k)] if d is not None}
    raw = {k: p.km.keyframe_pixels(s, k) for k in kfs}
    pts = p.km.download_points(s)
    point = {int(i): j for j, i in enumerate(pts["ids"])}
    rows = p.rows[s]
    live = {k: {int(i): tuple(px) for i, px, lv in zip(d["ids"], raw[k], d["live"]) if lv} for k, d in kfs.items()}
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
    frame = {"Tcw": nl.tcw_of(kfs[cur]["theta"]), "cam": p.cam, "cell_size": ls.CELL, "nb_3d_kpts": nb3}
    return (frame, keypoints, np.array([nl.tcw_of(kfs[k]["theta"]) for k in order]), local_map, ls.PARAMS), lm, kp_ids


def test_host_array_path_on_downloads_agrees(dev):
    """slam_local_map_match, which has always taken a lens, fed with downloads of the same map (the raw pixels from download_pixels) returns the pairs
    of the call staged on the device"""
    p = dev()
    for k in range(6):
        p.add()
        if k in ls.BA_AT:
            p.ba()
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


def test_without_the_store_a_lens_is_still_an_argument_error(dev, slam):
    p = dev(pixels=False)
    for k in range(3):
        p.add()
    with pytest.raises(slam.SlamHipError, match="distortion"):
        p.device_match()
    with pytest.raises(slam.SlamHipError, match="not enabled"):
        p.km.keyframe_pixels(0, 0)
    # a pinhole camera in the call: as ever, on the undistorted pixels the map has
    status, pairs, dist = p.km.local_map_match(ls.CAM10, ls.CELL, ls.PARAMS.max_projection_distance, ls.PARAMS.max_descriptor_distance)
    want = lz.LensRun.match(p, view="upx", lens=False)
    assert list(status) == [w["status"] for w in want] and 0 in status
    assert all(np.array_equal(pairs[s], want[s]["pairs"]) for s in range(S))


@pytest.mark.parametrize("mode", ms.MODES)
def test_zero_distortion_with_the_store_is_the_existing_path(dev, slam, mode):
    """a map with raw pixels and a pinhole camera beside a map without them, on kfmap_lmm_scripts' scenes with merges: every answer and every
    read-back of the two is the same, byte for byte, and the raw pixels are the slabs' own"""
    a, b = dev(dist=lz.ZERO, mode=mode), dev(dist=lz.ZERO, mode=mode, pixels=False)
    n = 0
    for k in range(ls.N_KF):
        mask = ls.LAST_MASK if k == ls.N_KF - 1 else None
        a.add(mask); b.add(mask)
        ra, rb = a.device_match(), b.device_match()
        want = lz.LensRun.match(a)
        assert list(ra[0]) == [w["status"] for w in want] and ra[0].tobytes() == rb[0].tobytes()
        for s in range(S):
            assert np.array_equal(ra[1][s], want[s]["pairs"]) and ra[1][s].tobytes() == rb[1][s].tobytes() and ra[2][s].tobytes() == rb[2][s].tobytes()
            da, db = a.km.debug_local_map(s), b.km.debug_local_map(s)
            assert all(np.asarray(da[key]).tobytes() == np.asarray(db[key]).tobytes() for key in da), s
            n += len(ra[1][s])
        a.merge(lz.pairs_of(want)); b.merge(lz.pairs_of(want))
        if k in ls.BA_AT:
            a.ba(); b.ba()
        a.check(); b.check()
        for s in range(S):
            for kf in range(max(a.nkf[s] - ls.R, 0), a.nkf[s]):
                da, db = a.km.download_keyframe(s, kf), b.km.download_keyframe(s, kf)
                assert (da is None) == (db is None)
                if da is not None:
                    assert all(da[key].tobytes() == db[key].tobytes() for key in da) and np.array_equal(a.km.keyframe_pixels(s, kf), da["upx"])
    assert n >= 30
