"""CPU: the bounded model of map_filtering! / remove_keyframe! (tests/np_kfmap_filter.py over tests/np_kfmap.py) on the scripted case both
filter test files run (np_kfmap_filter.STREAMS: 14 key-frames, after each one gather -> update -> filter).

First the coverage of the scripted case is asserted on the model's log -- every exit occurs, one `keep` sits exactly on the ratio -- then the
bounded model is held to its unbounded twin over tracked_ba.Record where nothing is forgotten (R = 16: no slot is re-used, ids < mcap), state
for state after every filter, and the gates and the update-after-filter rule are checked one by one."""
import numpy as np
import pytest

import kfmap_scripts as scr
import np_kfmap as km
import np_kfmap_filter as flt
import tracked_ba as tb
from test_kfmap_model_host import _orc_undistort, _same_state, _same_window


def _drive(R, with_record=False, stop=None):
    """The scripted case through the model (and the record); yields (s, k, m, rec, log, log_rec) after every filter."""
    for s, cfg in enumerate(flt.STREAMS):
        m = km.Map(flt.CAP, R, flt.MCAP, scr.CAM, None, flt.MINC, theta_fn=tb.theta_of, undistort_fn=_orc_undistort)
        rec = tb.Record(scr.CAM, None, flt.MINC, 0.0) if with_record else None
        for k, f in enumerate(flt.frames(cfg)[:stop]):
            lst = dict(ids=f["ids"], yx=f["yx"], is_3d=f["is_3d"], xyz=f["xyz"])
            km.add_keyframe(m, k, f["Tcw"], lst)
            wm = km.gather(m)
            if rec is not None:
                assert k < R and int(f["ids"].max()) < flt.MCAP, "nothing may be forgotten where the twin is compared"
                tb.add_keyframe(rec, k, f["Tcw"], lst)
                wr = tb.gather(rec)
                if wr is None or len(wr["poses_ids"]) == 0:
                    assert wm is None
                else:
                    _same_window(wr, wm)
            if wm is not None:
                ol, th = scr.outlier_pattern(cfg["seed"], wm), scr.refined(cfg["seed"], wm)
                km.update(m, wm, th, ol)
                if rec is not None:
                    tb.update(rec, wr, th, ol)
            log = flt.filter_map(m, cfg["ratio"], flt.MINC, flt.FIRST)
            log_rec = flt.filter_record(rec, cfg["ratio"], flt.MINC, flt.FIRST) if rec is not None else None
            yield s, k, m, rec, log, log_rec


def test_scripted_case_covers_every_exit():
    exits, on_the_ratio, reused = set(), 0, 0
    emptied = {}
    for s, k, m, rec, log, _ in _drive(8):
        for kfid, ex, n_total, n_good in log:
            exits.add(ex)
            assert (m.slot(kfid) is None) == (ex in ("few", "ratio")) or ex == "break"
            if ex in ("few", "ratio"):
                emptied[(s, kfid % 8)] = kfid
            on_the_ratio += ex == "keep" and n_total > 0 and n_good / n_total == flt.STREAMS[s]["ratio"]
        reused += emptied.get((s, k % 8)) == k - 8               # key-frame k was recorded into a slot the filter had emptied
        if s == 3:
            assert log == []                                     # ratio 1.0: the filter never acts
    assert exits == {"break", "keep", "few", "ratio"}, exits
    assert on_the_ratio >= 1 and reused >= 1


def test_bounded_model_equals_the_unbounded_twin_where_nothing_is_forgotten():
    removed = 0
    for s, k, m, rec, log, log_rec in _drive(16, with_record=True):
        assert log == log_rec, (s, k)
        _same_state(rec, m)
        removed += sum(ex in ("few", "ratio") for _, ex, _, _ in log)
    assert removed >= 2
    # ... and in the ring of 8 up to the key-frame that first re-uses a slot
    for s, k, m, rec, log, log_rec in _drive(8, with_record=True, stop=8):
        assert log == log_rec, (s, k)
        _same_state(rec, m)


def _hand_map(lists, R=4):
    m = km.Map(8, R, 64)
    for k, (ids, f3) in enumerate(lists):
        n = len(ids)
        km.add_keyframe(m, k, np.eye(4), dict(ids=np.array(ids, dtype=np.int64), yx=np.zeros((n, 2)), is_3d=np.array(f3, dtype=bool), xyz=np.zeros((n, 3))))
    return m


def test_gates():
    cfg = flt.STREAMS[0]
    m = next(m for s, k, m, rec, log, _ in _drive(8, stop=9) if s == 0 and k == 7)       # stream A before the key-frame whose filter removes two
    f = flt.frames(cfg)[8]
    km.add_keyframe(m, 8, f["Tcw"], f)
    before = (m.tag.copy(), list(m.mask))
    assert flt.filter_map(m, 1.0, flt.MINC, flt.FIRST) == [] and flt.filter_map(m, float("inf"), flt.MINC, flt.FIRST) == []      # ratio >= 1
    assert flt.filter_map(m, cfg["ratio"], flt.MINC, 9) == [] and flt.filter_map(m, cfg["ratio"], flt.MINC) == []                 # cur < first_kfid (default 20)
    assert np.array_equal(m.tag, before[0]) and list(m.mask) == before[1]
    assert any(ex == "ratio" for _, ex, _, _ in flt.filter_map(m, cfg["ratio"], flt.MINC, 8))                                    # cur == first_kfid acts
    # break at key-frame 0: it shares point 0 with the newest key-frame, so key-frame 1 (1 good of 1 at ratio 0) stays
    m = _hand_map([([0, 1], [1, 1]), ([0, 1], [1, 1]), ([0, 1], [1, 1])])
    assert flt.filter_map(m, 0.0, 0, 2) == [(0, "break", 0, 0)] and m.slot(1) is not None
    # 0 / 0 keeps: min_cov_score 1 (1 // 2 = 0: the `few` exit cannot fire), a candidate without a 3-D point
    m = _hand_map([([0, 1], [0, 0]), ([2, 3], [0, 0]), ([2, 3, 4], [0, 0, 0])])
    assert flt.filter_map(m, 0.0, 1, 2) == [(1, "keep", 0, 0)] and m.slot(1) is not None
    assert flt.filter_map(m, 0.0, 2, 2) == [(1, "few", 0, 0)] and m.slot(1) is None      # min_cov_score 2: 0 < 1
    # more than four observers, counted after the removals the call has already made: key-frames 1 .. 6 see point 9 (six observers, then five, then four)
    m = _hand_map([([0], [1])] + [([9], [1])] * 6, R=8)
    assert flt.filter_map(m, 0.0, 0, 2) == [(1, "ratio", 1, 1), (2, "ratio", 1, 1), (3, "keep", 1, 0), (4, "keep", 1, 0), (5, "keep", 1, 0)]


def test_remove_keyframe_of_the_model():
    m = _hand_map([([0, 1, 2], [1, 1, 0]), ([1, 2, 3], [1, 0, 1]), ([2, 3], [0, 1])])
    flt.remove_keyframe(m, 7)                                    # not in the ring: nothing
    assert [m.slot(k) for k in range(3)] == [0, 1, 2]
    with pytest.raises(ValueError):
        flt.remove_keyframe(m, 2)
    flags, xyz = m.flags.copy(), m.xyz.copy()
    flt.remove_keyframe(m, 1)
    assert m.slot(1) is None and m.n[1] == 0 and m.keyframe(1) is None
    assert [m.observers(m.entry(i)) for i in range(4)] == [[0], [0], [0, 2], [2]]
    assert np.array_equal(m.flags, flags) and np.array_equal(m.xyz, xyz)      # no is_bad evaluation, nothing else changes
    flt.remove_keyframe(m, 1)                                    # again: not in the ring


def test_update_after_filter_skips_the_removed_keyframe():
    """filtering between a gather and its update: the removed key-frame's pose is not copied and its outlier observations are not applied"""
    cfg = flt.STREAMS[2]                                         # stream C: the key-frame its filter removes at key-frame 8 has outlier observations in the window
    m = next(m for s, k, m, rec, log, _ in _drive(8, stop=9) if s == 2 and k == 7)
    f = flt.frames(cfg)[8]
    km.add_keyframe(m, 8, f["Tcw"], f)
    wm = km.gather(m)
    ol, th = scr.outlier_pattern(cfg["seed"], wm), scr.refined(cfg["seed"], wm)
    gone = [kfid for kfid, ex, _, _ in flt.filter_map(m, cfg["ratio"], flt.MINC, flt.FIRST) if ex in ("few", "ratio")]
    hit = [kfid for kfid in gone if kfid in wm["poses_remap"] and (ol & wm["obs_in_covmap"] & (wm["obs_kf"] == kfid)).any()]
    assert hit, "a removed key-frame must be a pose of the pending window with an outlier observation inside the covisibility map"
    slabs = {kfid: (m.ids[kfid % 8].copy(), m.live[kfid % 8].copy(), m.theta[kfid % 8].copy()) for kfid in gone}
    km.update(m, wm, th, ol)
    for kfid, (ids, live, theta) in slabs.items():
        b = kfid % 8
        assert m.slot(kfid) is None and m.tag[b] == -1
        assert np.array_equal(m.ids[b], ids) and np.array_equal(m.live[b], live) and np.array_equal(m.theta[b], theta)
    kept = [int(kf) for kf in wm["poses_remap"] if int(kf) not in gone]
    assert kept and all(np.array_equal(m.theta[m.slot(kf)], th[6 * i:6 * i + 6]) for i, kf in enumerate(wm["poses_remap"]) if int(kf) in kept)
    assert all(kfid not in m.observers(e) for e in range(m.mcap) if m.ptag[e] >= 0 for kfid in gone)
