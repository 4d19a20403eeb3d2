"""GPU: slam_kfmap_merge (csrc/kfmap_merge.inc) -- the pairs of a local-map match applied in HBM, the touched slabs and live lists rebuilt in id order --
against the model (tests/np_kfmap_merge.py) on the sequences of tests/kfmap_merge_scripts.py: S = 3, cap 64, R = 4, mcap = 128, eight key-frames, in
both modes (the lists follow the renames / later lists still carry the prev ids), and a hand-built case at cap = 300 whose renames cross the edge of a
256-record chunk.  tests/test_kfmap_merge_host.py shows that the sequences merge on every stream and hold a has_new skip, an equal-id tombstone and a
slab with several renames, and that the hand-built case holds a rename to the front, to the back, a 2-D prev, a non-3-D new, replaced and dead ids.

After EVERY step -- add_keyframe + add_descriptors, local_map_match, merge, the hand-picked merge, gather + update -- every key-frame of the ring
(download_keyframe), download_points and KeypointSet.download are array_equal to the model; the invariant (sorted, unique ids) is thereby tested
through use: the add_keyframe, gather / update(ks), filter and local_map_match that follow a merge search the rebuilt slabs and lists.  No tolerance
anywhere: the merge moves values, it computes none.  (A key-frame's angles are computed on the device in its own arithmetic; add() holds them to
1e-12 once, as tests/test_gpu_kfmap_filter.py does, and hands the device's bits to the model.)  The device side of every step and every comparison
are tests/kfmap_device.py's.  Every test fails without slam_kfmap_merge."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_device as kd  # noqa: E402
import kfmap_lmm_scripts as ls  # noqa: E402
import kfmap_merge_scripts as ms  # noqa: E402
import kfmap_scripts as scr  # noqa: E402
import np_kfmap as npk  # noqa: E402
import np_kfmap_filter as npf  # noqa: E402
import np_kfmap_merge as nm  # noqa: E402
from kfmap_device import check_map, device_bytes  # noqa: E402

pytestmark = pytest.mark.gpu
S = ls.S
EMPTY = np.zeros((0, 2), dtype=np.int64)


class Pair(kd.DeviceSide, ms.MergeRun):
    """the device map with its keypoint set beside the models, driven by the same scripted key-frames and descriptors"""


pair = kd.device_fixture(Pair, "pair")


@pytest.mark.parametrize("mode", ms.MODES)
def test_device_equals_model_after_every_step(pair, mode):
    p = pair(mode)
    seen = dict(applied=np.zeros(S, dtype=np.int64), idle=0, hand=[])

    def on_step(kind, k, data):
        p.check()
        if kind == "merge":
            seen["applied"] += p.dev_counts[:, 0]
        if kind == "hand":
            seen["hand"] += [k2 for ks_ in data[1] for k2 in ks_]

    # the sequence's merges take the pairs where the match left them on the device (pairs=None); the hand-picked ones are host pairs
    for k in range(ls.N_KF):
        last = k == ls.N_KF - 1
        on_step("add", k, p.add(ls.LAST_MASK if last else None))
        res = p.match()
        on_step("match", k, res)
        pairs = [r["pairs"] if r["status"] == 0 else EMPTY for r in res]
        idle = [s for s in range(S) if len(pairs[s]) == 0]
        before = p.device_bytes(idle, staged=False)
        p.merge(pairs, device_pairs=True)
        on_step("merge", k, pairs)
        if idle and len(idle) < S:                               # a stream without pairs beside streams with pairs: its bytes are what they were
            assert p.device_bytes(idle, staged=False) == before
            seen["idle"] += 1
        if k == ms.HAND_AT:
            hp, kinds = p.hand()
            p.merge(hp)
            on_step("hand", k, (hp, kinds))
        if k in ls.BA_AT:
            on_step("ba", k, p.ba())
    assert np.all(seen["applied"] >= 1) and seen["idle"] >= 1 and {"has_new", "tombstone"} <= set(seen["hand"])
    # a filter that removes, per stream, the covisible key-frame with the fewest 3-D points; then once more match and merge on what is left
    minc = []
    for s in range(S):
        log = npf.filter_map(copy.deepcopy(p.m[s]), 0.999999, 0, first_kfid=0)
        minc.append(2 * (min(t for _, _, t, _ in log) + 1) if log else 0)
    removed = p.km.filter(0.999999, np.array(minc, dtype=np.int32), first_kfid=0)
    logs = [npf.filter_map(p.m[s], 0.999999, minc[s], first_kfid=0) if p.sel[s] else [] for s in range(S)]
    assert [sorted(k for k, ex, _, _ in log if ex in ("few", "ratio")) for log in logs] == removed and sum(len(r) for r in removed) >= 1
    p.check()
    res = p.match()
    p.merge([r["pairs"] if r["status"] == 0 else EMPTY for r in res], device_pairs=True)
    p.check()


def test_device_pairs_equal_host_pairs(pair):
    a, b = pair("follow"), pair("follow")
    n = 0
    for k in range(6):
        for p in (a, b):
            p.add()
        ra, rb = a.match(), b.match()
        pairs = [r["pairs"] if r["status"] == 0 else EMPTY for r in ra]
        a.merge(pairs, device_pairs=True)
        b.merge(pairs, device_pairs=False)
        assert np.array_equal(a.dev_counts, b.dev_counts)
        assert a.device_bytes(range(S)) == b.device_bytes(range(S))
        n += int(a.dev_counts[:, 0].sum())
        if k in ls.BA_AT:
            a.ba(); b.ba()
    assert n >= 5
    # a match's pairs are consumed once: a second merge without a new match has no pairs and changes nothing
    before = a.device_bytes(range(S))
    assert not a.km.merge(a.ks).any() and a.device_bytes(range(S)) == before


def test_a_call_without_pairs_changes_nothing(pair):
    p = pair("follow")
    for k in range(5):
        p.add()
        p.match()
        if k in ls.BA_AT:
            p.ba()
    before = p.device_bytes(range(S))
    assert not p.km.merge(p.ks, [EMPTY] * S).any()
    assert p.km.merge(None, [EMPTY] * S, want_counts=False) is None
    p.km.ctx.synchronize()
    assert p.device_bytes(range(S)) == before
    status, pairs, dist = p.km.local_map_match(ls.CAM10, ls.CELL, ls.PARAMS.max_projection_distance, ls.PARAMS.max_descriptor_distance)
    want = ms.MergeRun.match(p)
    assert all(np.array_equal(pairs[s], want[s]["pairs"]) for s in range(S)) and sum(len(x) for x in pairs) >= 1      # the descriptors are where they were


def test_argument_errors_enqueue_nothing(pair, slam):
    p = pair("follow")
    for k in range(4):
        p.add()
        res = p.match()
        if k < 3:
            p.merge([r["pairs"] if r["status"] == 0 else EMPTY for r in res], device_pairs=True)
    pairs = [r["pairs"] if r["status"] == 0 else EMPTY for r in res]
    assert sum(len(x) for x in pairs) >= 2
    # a pending window (the reference merges under optimization_lock): device pairs and host pairs alike
    wins, status = p.km.gather(np.full(S, p.m[0].min_cov_score, dtype=np.int32))
    before = p.device_bytes(range(S))          # (behind the gather: it demotes is_bad points itself)
    busy = [w.stream for w in wins if len(pairs[w.stream])]
    assert busy
    with pytest.raises(slam.SlamHipError, match="pending"):
        p.km.merge(p.ks)
    with pytest.raises(slam.SlamHipError, match="pending"):
        p.km.merge(p.ks, pairs)
    free = [pairs[s] if s not in [w.stream for w in wins] else EMPTY for s in range(S)]
    # pairs that are not one-to-one: a prev twice, a new twice, an id on both sides; too many pairs; nothing for any stream
    s0 = busy[0]
    a, b = (int(v) for v in pairs[s0][0])
    for bad in ([(a, b), (a, b + 1)], [(a, b), (a + 1, b)], [(a, b), (b, a + 10 ** 6)]):
        arg = [np.array(bad, dtype=np.int64) if s == s0 else free[s] for s in range(S)]
        with pytest.raises(slam.SlamHipError, match="one-to-one"):
            p.km.merge(None, arg)
    with pytest.raises(slam.SlamHipError, match="pairs"):
        p.km.merge(None, [np.stack([np.arange(ls.CAP + 1), 10 ** 6 + np.arange(ls.CAP + 1)], axis=1)] + [EMPTY] * (S - 1))
    p.km.ctx.synchronize()
    assert p.device_bytes(range(S)) == before
    # the device-pairs path on a map without descriptors (there is no match whose pairs to take)
    plain = slam.KeyframeMap(S, ls.CAP, R=ls.R, mcap=ls.MCAP)
    try:
        with pytest.raises(slam.SlamHipError, match="not enabled"):
            plain.merge()
        assert not plain.merge(None, [EMPTY] * S).any()          # host pairs need no descriptors
    finally:
        plain.close()
    # behind the update the pending windows are gone and the match's pairs are still there: the merge equals the model's
    sol = ms.MergeRun.ba(p)
    p.km.update(wins, [sol[w.stream][1] for w in wins], [sol[w.stream][2] for w in wins], ks=p.ks)
    p.check()
    p.merge(pairs, device_pairs=True)
    p.check()
    assert p.dev_counts[:, 0].sum() + p.dev_counts[:, 1].sum() == sum(len(x) for x in pairs)


def test_the_hand_built_case_across_a_chunk_edge(slam):
    """cap = 300: the newest slab holds 286 records, the twenty redetections lie behind record 256 and land before it (HAND_PAIRS names every case);
    stream 0 has no pairs; every field of a list's record travels with its id; then the map is used: add_keyframe from the renamed lists as they lie
    in HBM, gather + update(ks), filter"""
    streams = ms.hand_streams()
    ks = slam.KeypointSet(S, ms.HCAP)
    km = slam.KeyframeMap(S, ms.HCAP, R=ms.HR, mcap=ms.HMCAP)
    models = [npk.Map(ms.HCAP, ms.HR, ms.HMCAP, ls.CAM10[:4], None, 8) for _ in range(S)]
    Tcw = np.tile(np.eye(4), (S, 1, 1))

    def record(k, lists=None):
        for s in range(S):
            f = streams[s][min(k, ms.HKF - 1)]
            Tcw[s] = f["Tcw"]
            if lists is None:
                ks.upload(s, f["yx"], f["is_3d"], f["xyz"], f["ids"])
            npk.add_keyframe(models[s], k, f["Tcw"], f if lists is None else lists[s])
        ks.keyframe()
        km.add_keyframe(ks, slam.stream_params(S, Tcw=Tcw, cam=ls.CAM10[:4], dist=np.zeros((S, 4))))
        for s in range(S):
            kd.hand_over_theta(km, models[s], s, k)
    try:
        for k in range(ms.HKF):
            record(k)
        lists = []
        for s in range(S):                                       # every field an upload can set, each value its own
            f, n = streams[s][-1], len(streams[s][-1]["ids"])
            extra = dict(kyx=f["yx"] + 1000.0 + s, has_kf=(f["ids"] % 3 != 0), first_yx=f["yx"] + 2000.0 + s, first_kf=(f["ids"] % 5).astype(np.int32))
            ks.upload_keyframe(s, extra["kyx"], extra["has_kf"])
            ks.upload_first(s, extra["first_yx"], extra["first_kf"], ms.HKF)
            lists.append(dict(ids=f["ids"].copy(), yx=f["yx"].copy(), is_3d=f["is_3d"].copy(), xyz=f["xyz"].copy(), **extra))
        check_map(km, ks, models, lists)
        nkf = [ms.HKF - 1] * S
        idle = device_bytes(km, ks, [0], nkf, staged=False)
        pairs = [EMPTY] + [np.array(ms.HAND_PAIRS, dtype=np.int64)] * (S - 1)
        want = np.zeros((S, 4), dtype=np.int32)
        for s in range(1, S):
            r = nm.merge(models[s], pairs[s], lists[s])
            lists[s] = r["list"]
            want[s] = (r["applied"], r["skipped"], r["renamed"], r["status"])
        got = km.merge(ks, pairs)
        assert np.array_equal(got, want) and tuple(got[1]) == (23, 3, got[1][2], 0) and got[1][2] >= 60
        check_map(km, ks, models, lists)
        assert device_bytes(km, ks, [0], nkf, staged=False) == idle
        for s in range(S):                                       # the fields the plain download does not show
            kyx, has_kf = ks.download_keyframe(s)
            fyx, fkf, count = ks.download_first(s)
            assert np.array_equal(kyx, lists[s]["kyx"]) and np.array_equal(has_kf, lists[s]["has_kf"]), s
            assert np.array_equal(fyx, lists[s]["first_yx"]) and np.array_equal(fkf, lists[s]["first_kf"]) and count == ms.HKF, s
            d = ks.download(s)
            assert not d["has_stereo"].any() and not d["stereo_yx"].any()
        # dead ids: every pair skipped, nothing changed
        before = device_bytes(km, ks, range(S), nkf, staged=False)
        got = km.merge(ks, [EMPTY] + [np.array(ms.HAND_DEAD, dtype=np.int64)] * (S - 1))
        assert np.array_equal(got[1:], [[0, 2, 0, 0]] * (S - 1)) and device_bytes(km, ks, range(S), nkf, staged=False) == before
        # through use: the next key-frame is recorded from the lists as the merge left them in HBM
        lists = [{key: l[key] for key in ("ids", "yx", "is_3d", "xyz")} for l in lists]
        record(ms.HKF, lists)
        check_map(km, ks, models, lists)
        wins, status = km.gather(np.full(S, 8, dtype=np.int32))
        assert [w.stream for w in wins] == list(range(S))
        sol = {}
        for s in range(S):
            win = npk.gather(models[s])
            theta, outl = scr.refined(40 + s, win), scr.outlier_pattern(40 + s, win)
            assert np.array_equal(wins[s].obs_kp, win["obs_kp"]) and np.array_equal(wins[s].obs_kf, win["obs_kf"]) and np.array_equal(wins[s].cache.pixels, win["pixels"])
            lists[s] = npk.update(models[s], win, theta, outl, lists[s])
            sol[s] = (theta, outl)
        km.update(wins, [sol[s][0] for s in range(S)], [sol[s][1] for s in range(S)], ks=ks)
        check_map(km, ks, models, lists)
        removed = km.filter(0.5, 8, first_kfid=0)
        logs = [npf.filter_map(models[s], 0.5, 8, first_kfid=0) for s in range(S)]
        assert [sorted(k for k, ex, _, _ in log if ex in ("few", "ratio")) for log in logs] == removed
        check_map(km, ks, models, lists)
    finally:
        km.close(); ks.close()
