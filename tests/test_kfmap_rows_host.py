"""CPU: the row model of the key-frame map (tests/np_kfmap_rows.py, the model of slam_kfmap_enable_descriptor_rows) against a literal restatement of
the reference's keyframes_descriptors, and what the scripted scenes (tests/kfmap_rows_scripts.py) hold.

  * the restatement (Point below) is written from map_point.jl:42-45 (the constructor), :88-146 (remove_kf_observation!, add_descriptor!), :165-174
    (mappoint_min_distance) and map_manager.jl:410-412 (merge_mappoints' copy) alone: a Dict kfid -> row per point, unbounded, beside
    tests/tracked_ba.py's Record.  With a ring and a table that forget nothing and D = 8 (dropped == 0) the model equals it after every step;
  * four mutants of the model are each rejected by that comparison;
  * on the model alone: the sequence yields a pair the one-row model does not find, the dropped counter becomes non-zero at D = 2 and stays zero
    at D = 4; the hand-built drift stream pairs C through B's row alone; the filter step of the GPU test has a point whose only observers are
    two removed key-frames."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_lmm_scripts as ls  # noqa: E402
import kfmap_merge_scripts as ms  # noqa: E402
import kfmap_rows_scripts as rs  # noqa: E402
import np_kfmap as npk  # noqa: E402
import np_kfmap_filter as npf  # noqa: E402
import np_kfmap_merge as nm  # noqa: E402
import np_kfmap_rows as nr  # noqa: E402


@pytest.fixture(autouse=True)
def entry_point():
    import slam_jl_amd
    from slam_jl_amd import _lib
    assert "slam_kfmap_enable_descriptor_rows" in _lib.SIGNATURES, "slam_kfmap_enable_descriptor_rows: the model has no entry point to describe"
    assert hasattr(slam_jl_amd.KeyframeMap, "descriptor_rows")


# ---- the literal restatement -----------------------------------------------------------------------------------------------------------------------------
class Point:
    """MapPoint as far as its descriptors go"""

    def __init__(self, kfid, descriptor):                        # map_point.jl:42-45
        self.observer_keyframes_ids = {kfid}
        self.descriptor = descriptor                             # (only its emptiness is read)
        self.keyframes_descriptors = {kfid: descriptor}


def remove_kf_observation(mp, kfid):                             # map_point.jl:88-122
    if kfid not in mp.observer_keyframes_ids:
        return
    mp.observer_keyframes_ids.remove(kfid)
    if not mp.observer_keyframes_ids:
        mp.descriptor = None
        mp.keyframes_descriptors.clear()
        return
    if kfid not in mp.keyframes_descriptors:
        return
    mp.keyframes_descriptors.pop(kfid)


def add_descriptor(mp, kfid, descriptor):                        # map_point.jl:124-146
    if kfid in mp.keyframes_descriptors:
        return
    mp.keyframes_descriptors[kfid] = descriptor
    if mp.descriptor is None or len(mp.keyframes_descriptors) == 1:
        mp.descriptor = descriptor


def mappoint_min_distance(m1, m2):                               # map_point.jl:165-174
    best = 1e6
    for d1 in m1.keyframes_descriptors.values():
        for d2 in m2.keyframes_descriptors.values():
            best = min(best, float(rs.hamming(d1, d2)))
    return best


def follow_record(rec, pts):
    """the Record's observer sets have changed: every observer a point lost goes through remove_kf_observation!, a removed point goes"""
    for i in [i for i in pts if i not in rec.mps]:
        del pts[i]
    for i, mp in pts.items():
        for kfid in sorted(mp.observer_keyframes_ids - rec.mps[i].obs):
            remove_kf_observation(mp, kfid)
        mp.observer_keyframes_ids |= rec.mps[i].obs              # add_keyframe_observation!


def same(rec, pts, m, D):
    """the model's rows against the restatement's, point for point"""
    got = nr.descriptor_rows(m, D)
    if list(got["ids"]) != sorted(rec.mps) or got["dropped"] != 0:
        return False
    for j, i in enumerate(int(i) for i in got["ids"]):
        mp = pts.get(i)
        want = {} if mp is None else mp.keyframes_descriptors
        if bool(got["described"][j]) != (mp is not None and mp.descriptor is not None):
            return False
        if [int(k) for k in got["keys"][j]] != sorted(want) or any(not np.array_equal(r, want[int(k)]) for k, r in zip(got["keys"][j], got["rows"][j])):
            return False
    return True


def _remove_obs(m, kp, kf):
    """remove_mappoint_obs! on the bounded map, as np_kfmap.update does it for an outlier observation"""
    b, e = m.slot(kf), m.entry(kp)
    m.live[b, m.find_live(b, kp)] = False
    m.mask[e] &= ~(1 << b)


def _same_key_pair(m, D, used):
    """two live 3-D points that both carry a row under one key and lie alive in one slab: the pair the equal-key skip is there for"""
    for b in range(m.R):
        if m.tag[b] < 0:
            continue
        ok = [int(m.ids[b, i]) for i in range(int(m.n[b])) if m.live[b, i] and m.entry(m.ids[b, i]) is not None and int(m.ids[b, i]) not in used
              and m.flags[int(m.ids[b, i]) % m.mcap] & npk.F_3D and int(m.tag[b]) in D["krows"][int(m.ids[b, i]) % m.mcap]]
        if len(ok) >= 2:
            return [(ok[0], ok[1])]
    return []


def _restatement_mismatches(mutant):
    """the scripted scenes on a ring and a table that forget nothing, D = 8: model and restatement step by step -> (comparisons that differ, counts)"""
    import tracked_ba as tb
    frames, descs, _ = rs.scenes()
    bad, seen = 0, dict(applied=0, equal_key=0, removed_obs=0, last=0, filtered=0, min_dist=0)
    for s in range(ls.S):
        m = npk.Map(ls.CAP, 16, 1024, ls.CAM10[:4])
        D = nr.new_descriptors(m, 8)
        rec, pts = tb.Record(ls.CAM10[:4]), {}
        for k, (f, d) in enumerate(zip(frames[s], descs[s])):
            nr.add_keyframe(m, D, k, f["Tcw"], f, mutant=mutant); nr.add_descriptors(m, D, d[0], d[1])
            tb.add_keyframe(rec, k, f["Tcw"], f)
            follow_record(rec, pts)
            for j, row in enumerate(d[1]):                       # add_mappoint!: a new point is made with the current key-frame's descriptor
                if d[0] + j in rec.mps and d[0] + j not in pts:
                    pts[d[0] + j] = Point(k, row)
            bad += not same(rec, pts, m, D)
            r = nr.local_map_match(m, D, ls.CAM10, ls.CELL, ls.PARAMS)
            for (a, b), dist in zip(r["pairs"], r["dist"]):     # the distance the match decided on is the minimum over all rows
                seen["min_dist"] += 1
                bad += dist != mappoint_min_distance(pts[int(a)], pts[int(b)])
            pairs = [(int(a), int(b)) for a, b in r["pairs"]]
            if k >= 2:
                pairs += ms.hand_pairs(m, avoid=[i for p in pairs for i in p])[0]
                pairs += _same_key_pair(m, D, set(i for p in pairs for i in p))
            if pairs:
                assert nm.check_pairs(pairs)
                for a, b in pairs:
                    prev = pts.get(a)
                    if nm.restated_merge(rec, a, b, with_list=False) is None:
                        continue
                    seen["applied"] += 1
                    if prev is not None:                         # map_manager.jl:410-412
                        seen["equal_key"] += b in pts and bool(set(prev.keyframes_descriptors) & set(pts[b].keyframes_descriptors))
                        for kfid, row in prev.keyframes_descriptors.items():
                            if b in pts:
                                add_descriptor(pts[b], kfid, row)
                            else:
                                pts[b] = Point(kfid, row); pts[b].observer_keyframes_ids = set()
                nr.merge(m, D, np.array(pairs, dtype=np.int64), None, with_list=False, mutant=mutant)
                follow_record(rec, pts)
                bad += not same(rec, pts, m, D)
            if k in (3, 5):                                      # outlier observations: every third live observation of key-frame k - 1 goes
                b = m.slot(k - 1)
                for i in range(0, int(m.n[b]), 3):
                    kp = int(m.ids[b, i])
                    if m.live[b, i] and m.entry(kp) is not None:
                        nr.through(_remove_obs)(m, D, kp, k - 1, mutant=mutant)
                        tb.remove_obs(rec, kp, k - 1)
                        seen["removed_obs"] += 1
                before = {i: bool(p.keyframes_descriptors) for i, p in pts.items()}
                follow_record(rec, pts)
                seen["last"] += sum(1 for i, p in pts.items() if before[i] and not p.observer_keyframes_ids)
                bad += not same(rec, pts, m, D)
        log = nr.filter_map(m, D, 0.5, 1000, first_kfid=0, mutant=mutant)           # every covisible key-frame but key-frame 0 goes
        log_rec = npf.filter_record(rec, 0.5, 1000, first_kfid=0)
        assert log == log_rec
        seen["filtered"] += sum(ex in ("few", "ratio") for _, ex, _, _ in log)
        before = {i: bool(p.keyframes_descriptors) for i, p in pts.items()}
        follow_record(rec, pts)
        seen["last"] += sum(1 for i, p in pts.items() if before[i] and not p.observer_keyframes_ids)
        bad += not same(rec, pts, m, D)
    return bad, seen


def test_model_equals_the_literal_restatement():
    bad, seen = _restatement_mismatches(None)
    assert bad == 0
    assert seen["applied"] >= 9 and seen["equal_key"] >= 1 and seen["removed_obs"] >= 10 and seen["last"] >= 1 and seen["filtered"] >= 3 and seen["min_dist"] >= 3, seen


@pytest.mark.parametrize("mutant", nr.MUTANTS)
def test_the_restatement_rejects_the_mutant(mutant):
    assert _restatement_mismatches(mutant)[0] >= 1


# ---- what the scenes hold, on the model alone ---------------------------------------------------------------------------------------------------------------
def _drift(max_rows):
    """the hand-built drift stream driven add -> match -> merge -> (found pairs, the run)"""
    frames, descs = rs.drift_stream()
    run = rs.RowsRun("follow", max_rows, frames=[frames], descs=[descs], seeds=(41,))
    found = []
    for k in range(rs.DRIFT_KF):
        run.add()
        res = run.match()
        found += [(k, int(a), int(b), float(d)) for a, b, d in zip(res[0]["pairs"][:, 0], res[0]["pairs"][:, 1], res[0]["dist"])] if res[0]["status"] == 0 else []
        run.merge([r["pairs"] if r["status"] == 0 else np.zeros((0, 2), dtype=np.int64) for r in res])
    return found, run


def test_the_drift_pair_needs_the_rows():
    with_rows, run = _drift(4)
    one_row, _ = _drift(None)
    assert (2, rs.DRIFT_B, rs.DRIFT_A, 60.0) in with_rows and (2, rs.DRIFT_B, rs.DRIFT_A, 60.0) in one_row
    assert (4, rs.DRIFT_C, rs.DRIFT_A, 60.0) in with_rows and not any(k == 4 and a == rs.DRIFT_C for k, a, _, _ in one_row)
    got = run.rows(0)
    j = list(got["ids"]).index(rs.DRIFT_A)
    assert list(got["keys"][j]) == [2, 4]                        # A's own row went with key-frame 0's slot: C paired through B's row alone


def test_the_scripted_sequence_pairs_more_with_rows_and_the_bound_drops_at_2_not_at_4():
    extra, dropped = 0, {}
    for mode in ms.MODES:
        base = set(rs.run_sequence(rs.RowsRun(mode, None)))
        for D in (2, 4):
            run = rs.RowsRun(mode, D)
            found = set(rs.run_sequence(run))
            dropped[mode, D] = [run.D[s]["dropped"] for s in range(rs.S)]
            extra += len(found - base)
    assert extra >= 1
    assert all(v == 0 for mode in ms.MODES for v in dropped[mode, 4]), dropped
    assert any(v > 0 for mode in ms.MODES for v in dropped[mode, 2]), dropped


def test_the_filter_step_has_a_point_whose_only_observers_are_two_removed_keyframes():
    n = 0
    for mode in ms.MODES:
        run = rs.RowsRun(mode, 4)
        before = {}

        def on_step(kind, k, data):
            if kind == "merge" and k == ls.N_KF - 1:
                before["m"] = [copy.deepcopy(m) for m in run.m]
            if kind == "filter":
                for s, log in enumerate(data):
                    n_ = rs.orphaned_by_filter(before["m"][s], [kf for kf, ex, _, _ in log if ex in ("few", "ratio")])
                    before.setdefault("n", []).append(len(n_))
        rs.run_sequence(run, on_step)
        n += sum(before["n"])
    assert n >= 1
