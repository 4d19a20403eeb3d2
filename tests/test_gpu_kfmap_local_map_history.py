"""GPU: slam_kfmap_local_map_match with the local-map history (slam_kfmap_enable_local_map_history, k_kfm_lm_stage_hist in csrc/kfmap_lmm.inc) against
the model (tests/np_kfmap_local_map_history.py) on the main scene of tests/kfmap_history_scripts.py: S = 3, cap 64, R = 6, mcap = 128, 12 key-frames, the
match's pairs merged where they lie on the device, a local-BA update behind key-frames 3 and 4, one filter.  tests/test_kfmap_local_map_history_host.py
shows that the scene has, on every stream, pairs that only the chain of stored local maps brings, purged ids, re-used slots and margins >= 1e-9.

After EVERY step the status, pairs, distances, the staged lists, the stored set of every key-frame of the ring (local_map_ids), every key-frame
(download_keyframe) and the points (download_points) are array_equal to the model, proj_yx included.  A key-frame's angles are computed on the device;
add() holds them to 1e-12 once and hands the device's bits to the model.  The device side of every step and every comparison are
tests/kfmap_device.py's.  Every test that enables the history fails without slam_kfmap_enable_local_map_history."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_device as kd  # noqa: E402
import kfmap_history_scripts as hs  # noqa: E402
import kfmap_lmm_scripts as ls  # noqa: E402
import np_kfmap_filter as npf  # noqa: E402
import np_kfmap_local_map_history as nh  # noqa: E402

pytestmark = pytest.mark.gpu
S = hs.S
FILTER_AT = 9


class Pair(kd.DeviceSide, hs.HistoryRun):
    """the device map with its keypoint set beside the models, driven by the same scripted key-frames and descriptors"""
    device_pairs = True                                          # merge(): the model's of `pairs`, the device's of the pairs its last match left in HBM

    def __init__(self, slam, history=True, mcap=hs.MCAP, **kw):
        super().__init__(slam, history=history, mcap=mcap, lm_history=history, **kw)

    def device_sets(self, s):
        """{kfid: stored set, or the error's text} of every key-frame id the ring can hold"""
        return {k: kd.stored_set(self.km, s, k) for k in range(max(self.nkf[s] - hs.R, 0), self.nkf[s])}

    def remove_keyframe(self, s, kfid):
        super().remove_keyframe(s, kfid)
        self.km.remove_keyframe(s, kfid)

    def reset(self, s):
        super().reset(s)
        self.km.reset(s)


pair = kd.device_fixture(Pair, "pair")


def _filter(p):
    """a filter that removes, per stream, the covisible key-frame with the fewest 3-D points (np_kfmap_filter's rule `n_total < min_cov_score / 2`)"""
    minc = []
    for s in range(S):
        log = npf.filter_map(copy.deepcopy(p.m[s]), 0.999999, 0, first_kfid=0)
        minc.append(2 * (min(t for _, _, t, _ in log) + 1) if log else 0)
    removed = p.km.filter(0.999999, np.array(minc, dtype=np.int32), first_kfid=0)
    logs = [npf.filter_map(p.m[s], 0.999999, minc[s], first_kfid=0) for s in range(S)]
    assert [sorted(k for k, ex, _, _ in log if ex in ("few", "ratio")) for log in logs] == removed and sum(len(r) for r in removed) >= 1


def test_device_equals_model_after_every_step(pair):
    p = pair()
    seen = dict(outside=[0] * S, pairs=0, steps=set())

    def on_step(kind, k, data):
        p.check()
        seen["steps"].add(kind)
        if kind == "match":
            for s, r in enumerate(data):
                seen["outside"][s] += sum(1 for q in r["pairs"] if int(q[1]) not in set(r["C"]))
                seen["pairs"] += len(r["pairs"])
        if kind == "merge" and k == FILTER_AT:
            _filter(p)
            p.check()
    hs.run_sequence(p, on_step=on_step)
    assert min(seen["outside"]) >= 1 and seen["pairs"] >= 60 and seen["steps"] == {"add", "match", "merge", "ba"}
    assert all(h.count["purged"] >= 10 and h.count["chained"] >= 3 for h in p.H)


def test_history_off_on_the_same_scene_is_the_parents_match(pair):
    p = pair(history=False)
    n = 0

    def on_step(kind, k, data):
        nonlocal n
        if kind == "match":
            n += sum(len(r["pairs"]) for r in data)
    hs.run_sequence(p, on_step=on_step)
    assert n >= 60
    with pytest.raises(p.slam.SlamHipError, match="not enabled"):
        p.km.local_map_ids(0, p.nkf[0] - 1)


@pytest.mark.parametrize("want", ("union", "replace"))
def test_a_second_match_for_one_key_frame_takes_the_rules_branch(pair, want):
    p = pair()
    hs.run_sequence(p, n_kf=hs.TWO_CALLS_AT + 1)
    plans = [hs.plan_second_call(p, s, want) for s in range(S)]
    assert all(plans)
    for s, drop in enumerate(plans):
        for k in drop:
            p.remove_keyframe(s, k)
    p.check()
    res = p.match()
    assert all(r["branch"] == want for r in res)
    p.check()
    again = p.match()                                              # and once more on the unchanged map: the same results, the same sets
    assert all(np.array_equal(a["pairs"], b["pairs"]) and np.array_equal(a["lm_ids"], b["lm_ids"]) for a, b in zip(res, again))


def test_an_unselected_stream_keeps_its_sets_and_bytes(pair):
    p = pair()
    hs.run_sequence(p, n_kf=7)
    before = p.device_bytes([1])
    p.add((1, 0, 1))
    res = p.match()
    assert res[1]["status"] == 1 and res[0]["status"] == 0 and res[2]["status"] == 0
    assert p.device_bytes([1]) == before and len(p.km.local_map_ids(1, 6)) >= 1
    p.check()


def test_a_key_frame_whose_match_was_skipped_gives_the_chain_nothing(pair):
    p = pair()
    skipped, met = (6, 7), 0
    for k in range(hs.N_KF):
        p.add()
        if k in skipped:
            continue
        oldest = [min(hs.covisible_ids(p, s), default=-1) for s in range(S)]
        res = p.match()
        for s in range(S):
            if oldest[s] in skipped:
                met += 1
                assert res[s]["chain"] == [] and p.H[s].kf[oldest[s] % hs.R] != oldest[s]
                with pytest.raises(p.slam.SlamHipError, match="no local map was stored"):
                    p.km.local_map_ids(s, oldest[s])
        p.merge(hs.pairs_of(res))
        if k in hs.BA_AT:
            p.ba()
    assert met >= 2
    p.check()


def test_status_2_still_stores_the_set_and_max_local_mcap_rules_it_out(pair):
    p = pair()
    hs.run_sequence(p, n_kf=8)
    p.add()
    dry = p.match()
    sizes = [len(r["lm_ids"]) for r in dry]
    big = int(np.argmax(sizes))
    assert sizes[big] >= 2 and dry[big]["status"] == 0
    # the largest bound that is too small (the bound also decides whether the chain runs, so it is asked of the model, on a copy of the history)
    status_at = lambda v: nh.local_map_match(p.m[big], p.D[big], copy.deepcopy(p.H[big]), ls.CAM10, ls.CELL, ls.PARAMS, max_local=v)["status"]
    ml = max(v for v in range(1, sizes[big]) if status_at(v) == 2)
    res = p.match(max_local=ml)                                    # (check_match compares the stored sets too)
    assert res[big]["status"] == 2 and len(p.km.debug_local_map(big)["lm_ids"]) == 0
    assert len(p.km.local_map_ids(big, p.nkf[big] - 1)) > ml
    full = p.match(max_local=hs.MCAP)
    assert all(r["status"] != 2 for r in full)
    p.check()


def test_reset_clears_one_streams_history(pair):
    p = pair()
    hs.run_sequence(p, n_kf=8)
    others = p.device_bytes([0, 2])
    assert not isinstance(p.device_sets(1)[7], str)
    p.reset(1)
    assert all(isinstance(v, str) for v in p.device_sets(1).values()) and p.device_bytes([0, 2]) == others
    for k in range(8, hs.N_KF):                                    # the stream starts anew beside the others
        p.add()
        res = p.match()
        p.merge(hs.pairs_of(res))
    p.check()
    assert all(isinstance(v, str) == (k < 8) for k, v in p.device_sets(1).items())


def test_enabling_twice_is_a_no_op(pair):
    p = pair()
    hs.run_sequence(p, n_kf=7)
    before = p.device_bytes(range(S))
    p.km.enable_local_map_history()
    assert p.device_bytes(range(S)) == before
    p.add()
    p.match()
    p.check()


def test_download_errors_and_errors_enqueue_nothing(pair, slam):
    p = pair()
    hs.run_sequence(p, n_kf=8)
    before = p.device_bytes(range(S))
    cur = p.nkf[0] - 1
    with pytest.raises(slam.SlamHipError, match="not in the ring"):
        p.km.local_map_ids(0, cur + 1)                             # never added
    with pytest.raises(slam.SlamHipError, match="not in the ring"):
        p.km.local_map_ids(0, cur - hs.R)                          # forgotten: its slot holds a newer key-frame
    with pytest.raises(slam.SlamHipError):
        p.km.local_map_ids(S, cur)
    n = len(p.km.local_map_ids(0, cur))
    assert n >= 2
    ids = np.zeros(n - 1, dtype=np.int64)
    import ctypes as C
    from slam_jl_amd import _lib as L
    cnt = C.c_int32(0)
    rc = p.km.ctx.lib.slam_kfmap_download_local_map_ids(p.km.ctx.h, p.km.h, 0, cur, L.ptr(ids, L.i64p), n - 1, C.byref(cnt))
    assert rc != 0 and cnt.value == n
    with pytest.raises(slam.SlamHipError, match="cap_ids"):
        p.km.ctx.check(rc)
    cam = np.tile(np.array(ls.CAM10), (S, 1))
    cam[1, 6] = 1e-4
    with pytest.raises(slam.SlamHipError, match="distortion"):     # an argument error of the match: no purge, no store, nothing staged
        p.km.local_map_match(cam, ls.CELL, 2.0, 0.35)
    assert p.device_bytes(range(S)) == before
    plain = slam.KeyframeMap(S, hs.CAP, R=hs.R, mcap=hs.MCAP)
    try:
        with pytest.raises(slam.SlamHipError, match="not enabled"):
            plain.local_map_ids(0, 0)
    finally:
        plain.close()


def test_a_table_whose_size_is_no_multiple_of_64(pair):
    """mcap = 100: the last word of every set is partial"""
    p = pair(mcap=100)
    n = 0

    def on_step(kind, k, data):
        nonlocal n
        if kind == "match":
            n += sum(len(r["pairs"]) for r in data)
        if kind in ("match", "ba"):
            p.check()
    hs.run_sequence(p, on_step=on_step)
    assert n >= 30 and all(h.count["purged"] >= 10 for h in p.H)
