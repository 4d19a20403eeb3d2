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
1e-12 once and hands the device's bits to the model.  The device side of every step and every comparison are tests/kfmap_device.py's; this file
passes it the tolerances above.  Every test fails without slam_kfmap_enable_pixels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_device as kd  # noqa: E402
import kfmap_lens_scripts as lz  # noqa: E402
import kfmap_lmm_scripts as ls  # noqa: E402
import kfmap_merge_scripts as ms  # noqa: E402

pytestmark = pytest.mark.gpu
S = ls.S


class Dev(kd.DeviceSide, lz.LensRun):
    """the device map with its keypoint set beside the models, driven by the same scripted key-frames and descriptors; pixels=False: a map that
    never enables the raw pixels"""
    device_pairs = True                                          # merge(): the model's of `pairs`, the device's of the pairs its last match left in HBM
    upx_tol = px_tol = kd.PX_TOL                                 # the slabs' and windows' undistorted pixels: the device's undistort_px may contract multiply-adds
    proj_tol = kd.PX_TOL                                         # staged proj_yx: projected through the lens in the device's own arithmetic

    def __init__(self, slam, dist=lz.DIST, mode="stale", kind="plain", pixels=True):
        super().__init__(slam, dist=dist, mode=mode, kind=kind, descriptor_rows=2 if kind == "rows" else None, lm_history=kind == "history")
        if pixels:
            self.km.enable_pixels()
            self.km.enable_pixels()                              # a second call is a no-op
        self.has_pixels = pixels


dev = kd.device_fixture(Dev, "dev")


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
