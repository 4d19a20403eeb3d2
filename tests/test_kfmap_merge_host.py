"""CPU: the model of slam_kfmap_merge (tests/np_kfmap_merge.py) on the sequences of tests/kfmap_merge_scripts.py.

  * independence: where nothing is forgotten (a ring and a table larger than the sequence) the model equals a sequential dict-and-set restatement of
    merge_mappoints (src/map_manager.jl:378-427) on tests/tracked_ba.py's unbounded Record, whatever the order the pairs are applied in;
  * the sequences the GPU tests run (S = 3, cap 64, R = 4, mcap = 128, both modes) actually merge: at least one pair applied on every stream, and over
    the whole sequence a has_new skip, an equal-id tombstone and a slab with several renames; every slab and list stays sorted;
  * the hand-built case at cap = 300 holds what its pairs are there for (front, back, across the 256-record chunk edge, 2-D prev, skipped pairs);
  * mutants: each of four broken rules changes a state;
  * the edges of the rules, one by one.
The model describes an entry point of the library: every test here first asserts that it exists."""
import copy
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_lmm_scripts as ls  # noqa: E402
import kfmap_merge_scripts as ms  # noqa: E402
import np_kfmap as npk  # noqa: E402
import np_kfmap_local_map as nl  # noqa: E402
import np_kfmap_merge as nm  # noqa: E402


@pytest.fixture(autouse=True)
def entry_point():
    import slam_jl_amd
    from slam_jl_amd import _lib
    assert "slam_kfmap_merge" in _lib.SIGNATURES, "slam_kfmap_merge: the model has no entry point to describe"
    assert hasattr(slam_jl_amd.KeyframeMap, "merge")


def _lst(ids, is_3d=None, xyz=None, yx=None):
    n = len(ids)
    return dict(ids=np.array(ids, dtype=np.int64), yx=np.arange(2.0 * n).reshape(n, 2) + 5.0 if yx is None else np.asarray(yx, dtype=np.float64),
                is_3d=np.ones(n, dtype=bool) if is_3d is None else np.array(is_3d, dtype=bool),
                xyz=np.arange(3.0 * n).reshape(n, 3) + 100.0 * np.array(ids, dtype=np.float64)[:, None] if xyz is None else np.asarray(xyz, dtype=np.float64))


def _same_as_record(rec, m, with_gone):
    for kfid, kf in rec.kfs.items():
        mk = m.keyframe(kfid)
        assert mk is not None and np.all(np.diff(mk["ids"]) > 0), kfid
        px = {int(i): (float(p[0]), float(p[1])) for i, p, l in zip(mk["ids"], mk["upx"], mk["live"]) if l}
        assert px == kf.px, kfid
    pts = m.points()
    assert list(pts["ids"]) == sorted(rec.mps)
    for j, i in enumerate(pts["ids"]):
        mp = rec.mps[int(i)]
        assert pts["observers"][j] == tuple(sorted(mp.obs)) and np.array_equal(pts["xyz"][j], mp.xyz), i
        assert (pts["is_3d"][j], pts["observed"][j]) == (mp.is_3d, mp.observed), i
    if with_gone:
        assert m.gone() == tuple(sorted(rec.gone))


@pytest.mark.parametrize("mode", ms.MODES)
def test_model_equals_the_sequential_restatement_in_any_order(mode):
    import tracked_ba as tb
    follow = mode == "follow"
    frames, descs = ls.scenes()
    applied_total, multi = 0, 0
    for s in range(ls.S):
        m = npk.Map(ls.CAP, 16, 1024, ls.CAM10[:4])
        D = nl.new_descriptors(m)
        rec = tb.Record(ls.CAM10[:4])
        ren = {}
        for k, (f, d) in enumerate(zip(frames[s], descs[s])):
            if follow:                                           # the lists follow the renames
                ids, have = [], set(int(i) for i in f["ids"])
                for i in (int(i) for i in f["ids"]):
                    j = i
                    while j in ren:
                        j = ren[j]
                    j = i if j != i and j in have else j         # (the list carries the new id too: prev stays)
                    have.add(j); ids.append(j)
                order = np.argsort(np.array(ids, dtype=np.int64), kind="stable")
                f = dict(Tcw=f["Tcw"], ids=np.array(ids, dtype=np.int64)[order], yx=f["yx"][order], is_3d=f["is_3d"][order], xyz=f["xyz"][order])
            nl.add_keyframe(m, D, k, f["Tcw"], f); nl.add_descriptors(m, D, d[0], d[1])
            tb.add_keyframe(rec, k, f["Tcw"], f)
            _same_as_record(rec, m, not follow)
            r = nl.local_map_match(m, D, ls.CAM10, ls.CELL, ls.PARAMS)
            pairs = [(int(a), int(b)) for a, b in r["pairs"]]
            if k >= 2:                                           # and pairs the match cannot produce: two ids alive in one slab
                hp, _ = ms.hand_pairs(m, avoid=[i for p in pairs for i in p])
                pairs += hp
            if not pairs:
                continue
            assert nm.check_pairs(pairs)
            shuffles = []
            for t in range(4):
                order = list(pairs)
                random.Random(100 * s + 10 * k + t).shuffle(order)
                rc = copy.deepcopy(rec)
                n = [nm.restated_merge(rc, a, b, with_list=follow) for a, b in order]
                shuffles.append((tb.snapshot(rc)[2:], {kf: dict(v.px) for kf, v in rc.kfs.items()}, sorted(x for x in n if x is not None), rc))
            for sh in shuffles[1:]:                              # the merges commute
                assert sh[:3] == shuffles[0][:3], (s, k)
            log = {}
            out = nm.merge(m, np.array(pairs, dtype=np.int64), _lst(f["ids"], f["is_3d"], f["xyz"], f["yx"]) if follow else None, with_list=follow, log=log)
            rec = shuffles[0][3]
            _same_as_record(rec, m, not follow)
            assert out["applied"] == len(shuffles[0][2]) and out["renamed"] == sum(shuffles[0][2]) and out["skipped"] == len(pairs) - out["applied"]
            assert nm.sorted_unique(m)
            applied_total += out["applied"]; multi += log["multi"]
            if follow:
                ren.update({a: b for a, b in pairs if m.entry(a) is None and a not in ren})
                assert np.all(np.diff(out["list"]["ids"]) > 0) and len(out["list"]["ids"]) == len(f["ids"])
    assert applied_total >= 9 and multi >= 1


def _sequence(mode, mutant=None):
    run = ms.MergeRun(mode)
    steps, applied, hand_kinds = [], np.zeros(ls.S, dtype=np.int64), []

    def on_step(kind, k, data):
        steps.append((kind, k, [nm.snapshot(m) for m in run.m], [None if l is None else {a: v.tobytes() for a, v in l.items()} for l in run.lists]))
        if kind in ("merge", "hand"):
            applied[:] += run.counts[:, 0]
            if mutant is None:
                assert all(nm.sorted_unique(m) for m in run.m), (kind, k)
                assert all(l is None or np.all(np.diff(l["ids"]) > 0) for l in run.lists), (kind, k)
        if kind == "hand":
            hand_kinds.extend(k2 for ks in data[1] for k2 in ks)
    ms.run_sequence(run, on_step, mutant=mutant)
    return run, steps, applied, hand_kinds


@pytest.mark.parametrize("mode", ms.MODES)
def test_the_gpu_sequences_actually_merge(mode):
    run, steps, applied, hand_kinds = _sequence(mode)
    assert np.all(applied >= 1), applied                        # at least one pair applied on every stream
    total = {key: sum(log.get(key, 0) for log in run.log) for key in ("has_new", "tombstone", "multi")}
    assert all(v >= 1 for v in total.values()), total
    assert {"has_new", "tombstone"} <= set(hand_kinds)
    assert all(run.nkf[s] > ls.R for s in range(ls.S))           # the ring has wrapped
    if mode == "stale":                                          # later lists still carry the prev ids: gone and dead, recorded as tombstones
        n_dead = 0
        for s in range(ls.S):
            m = run.m[s]
            for a in run.ren[s]:
                e = a % m.mcap
                if m.ptag[e] == a:
                    assert m.flags[e] & npk.F_DEAD and m.flags[e] & npk.F_GONE
                    n_dead += any(a in m.ids[b, :int(m.n[b])] and not m.live[b, list(m.ids[b, :int(m.n[b])]).index(a)] for b in range(m.R))
        assert n_dead >= 1
    else:                                                        # the lists followed: a renamed id is observed again by later key-frames
        assert sum(len(r) for r in run.ren) >= 3
        seen_again = 0
        for s in range(ls.S):
            m = run.m[s]
            for b in set(run.ren[s].values()):
                e = m.entry(b)
                seen_again += e is not None and bin(m.mask[e]).count("1") >= 2
        assert seen_again >= 1


def _hand_run(with_list, mutant=None):
    frames = ms.hand_scene()
    m = npk.Map(ms.HCAP, ms.HR, ms.HMCAP, ls.CAM10[:4])
    for k, f in enumerate(frames):
        npk.add_keyframe(m, k, f["Tcw"], f)
    lst = _lst(frames[-1]["ids"], frames[-1]["is_3d"], frames[-1]["xyz"], frames[-1]["yx"]) if with_list else None
    log = {}
    before = copy.deepcopy(m)
    out = nm.merge(m, np.array(ms.HAND_PAIRS, dtype=np.int64), lst, with_list=with_list, mutant=mutant, log=log)
    return frames, before, m, out, log


def test_the_hand_built_case_holds_its_cases():
    frames, before, m, out, log = _hand_run(True)
    assert (out["applied"], out["skipped"], out["status"]) == (23, 3, 0) and nm.sorted_unique(m)
    assert log["front"] >= 1 and log["back"] >= 2 and log["multi"] >= 3 and log["has_new"] == 1 and log["flat_prev"] == 1 and log["tombstone"] == 0
    # across the chunk edge: in the newest slab the twenty redetections lay behind record 256 and land before it
    b = 4 % ms.HR
    was = {int(i): j for j, i in enumerate(before.ids[b, :int(before.n[b])])}
    now = {int(i): j for j, i in enumerate(m.ids[b, :int(m.n[b])])}
    assert int(before.n[b]) > 256 and all(was[400 + j] >= 256 and now[100 + j] < 256 for j in range(20)) and int(m.n[b]) == int(before.n[b])
    assert now[3] == 0                                           # to the front
    b2 = 2 % ms.HR
    assert int(m.ids[b2, int(m.n[b2]) - 1]) == 500               # to the back
    # the has_new skip left an orphan: key-frame 1 still holds 50 alive, the point is gone
    assert m.find_live(1, 50) is not None and m.find_live(1, 500) is not None and m.entry(50) is None
    assert m.observers(m.entry(500)) == [1, 2, 3, 4] and m.flags[500 % ms.HMCAP] & npk.F_OBS
    # id 50 was observed by key-frame 0, whose slot key-frame 4 has taken: the bit of that slot now means key-frame 4
    assert 50 in frames[0]["ids"] and before.tag[0] == 4
    # the skipped pairs changed nothing of theirs
    for a, b_ in ((422, 5), (423, 2000), (424, 6)):
        assert m.entry(a) is not None and m.find_live(0, a) is not None
    assert m.ptag[6] == 1030
    # the list: renamed slots carry the new id, is_3d and the map's position; every other field travelled
    lst = out["list"]
    src = {int(i): j for j, i in enumerate(frames[-1]["ids"])}
    assert np.all(np.diff(lst["ids"]) > 0) and len(lst["ids"]) == len(frames[-1]["ids"])
    ren = {a: b_ for a, b_ in ms.HAND_PAIRS[:23]}
    back = {b_: a for a, b_ in ren.items()}
    for j, i in enumerate(int(i) for i in lst["ids"]):
        o = src[back.get(i, i)]
        assert np.array_equal(lst["yx"][j], frames[-1]["yx"][o])
        if i in back:
            assert lst["is_3d"][j] and np.array_equal(lst["xyz"][j], m.xyz[i % ms.HMCAP])
        else:
            assert lst["is_3d"][j] == frames[-1]["is_3d"][o] and np.array_equal(lst["xyz"][j], frames[-1]["xyz"][o])
    assert lst["is_3d"][list(lst["ids"]).index(4)] and not frames[-1]["is_3d"][src[421]]      # the 2-D prev became 3-D with the new point
    # a second call with dead ids: every pair skipped, nothing changed
    snap = nm.snapshot(m)
    out2 = nm.merge(m, np.array(ms.HAND_DEAD, dtype=np.int64), None, with_list=True)
    assert (out2["applied"], out2["skipped"]) == (0, 2) and nm.snapshot(m) == snap


def test_each_mutant_changes_a_state():
    true_seq = {mode: _sequence(mode)[1] for mode in ms.MODES}
    true_hand = nm.snapshot(_hand_run(True)[2])
    for mu in nm.MUTANTS:
        changed = []
        for mode in ms.MODES:
            steps = _sequence(mode, mutant=mu)[1]
            changed += [(mode, a[0], a[1]) for a, b in zip(steps, true_seq[mode]) if a[2:] != b[2:]]
        if nm.snapshot(_hand_run(True, mutant=mu)[2]) != true_hand:
            changed.append("hand")
        assert changed, f"no sequence tells the mutant `{mu}` from the model"
    # each mutant is told by the case made for it
    _, _, m, out, _ = _hand_run(True, mutant="flat")
    assert out["applied"] == 24 and m.entry(422) is None         # merged into the 2-D point 5
    _, _, m, _, _ = _hand_run(True, mutant="has_new")
    assert m.find_live(1, 50) is None                            # key-frame 1 then holds id 500 twice
    _, _, m, _, _ = _hand_run(True, mutant="unsorted")
    assert not nm.sorted_unique(m)


def _small():
    """R = 4, mcap = 8, cap = 8: key-frame 0 sees 1 2 3, key-frame 1 sees 2 3 4 (4 is 2-D), key-frame 2 sees 3 5"""
    m = npk.Map(8, 4, 8, ls.CAM10[:4])
    npk.add_keyframe(m, 0, np.eye(4), _lst([1, 2, 3]))
    npk.add_keyframe(m, 1, np.eye(4), _lst([2, 3, 4], is_3d=[True, True, False]))
    npk.add_keyframe(m, 2, np.eye(4), _lst([3, 5]))
    return m


def test_the_rules_one_by_one():
    # a plain merge: 5 (key-frame 2) into 1 (key-frame 0)
    m = _small()
    xyz1, upx5 = m.xyz[1].copy(), m.upx[2, 1].copy()
    out = nm.merge(m, [(5, 1)], _lst([3, 5]))
    assert (out["applied"], out["skipped"], out["renamed"]) == (1, 0, 1)
    assert list(m.ids[2, :2]) == [1, 3] and np.array_equal(m.upx[2, 0], upx5) and m.live[2, 0]          # moved to its place, pixel and live byte kept
    assert m.entry(5) is None and m.flags[5] == npk.F_DEAD and m.observers(m.entry(1)) == [0, 2]
    assert m.flags[1] & npk.F_OBS and np.array_equal(m.xyz[1], xyz1) and not m.flags[1] & npk.F_BA
    assert list(out["list"]["ids"]) == [1, 3] and np.array_equal(out["list"]["xyz"][0], xyz1) and np.array_equal(out["list"]["yx"][0], _lst([3, 5])["yx"][1])
    # without a list prev is also gone: a later list that still carries 5 does not record it
    m = _small()
    nm.merge(m, [(5, 1)], None)
    assert m.flags[5] == npk.F_DEAD | npk.F_GONE
    npk.add_keyframe(m, 3, np.eye(4), _lst([3, 5, 6]))
    assert m.entry(5) is None and m.find_live(3, 5) is None and list(m.ids[3, :3]) == [3, 5, 6]
    # validity: equal ids, a 2-D new point, an id that is not there, ids that share a table entry (only one of them is present)
    for pair in ((3, 3), (5, 4), (5, 7), (5, 13), (13, 1)):
        m = _small()
        snap = nm.snapshot(m)
        out = nm.merge(m, [pair], None)
        assert (out["applied"], out["skipped"]) == (0, 1) and nm.snapshot(m) == snap, pair
    # has_new: key-frame 1 holds 2 and 3; 2 -> 3 renames key-frame 0? it holds both as well: nothing is renamed, 2 dies, its observations are orphans
    m = _small()
    out = nm.merge(m, [(2, 3)], None)
    assert (out["applied"], out["renamed"]) == (1, 0) and m.find_live(0, 2) is not None and m.find_live(1, 2) is not None and m.entry(2) is None
    # a tombstone of the arriving id is dropped, another tombstone stays: key-frame 1 holds 2 (tombstone), 3 (tombstone), 4
    m = _small()
    m.live[1, 0] = False; m.mask[2] &= ~2; m.live[1, 1] = False; m.mask[3] &= ~2
    out = nm.merge(m, [(4, 2)], None)
    assert out["renamed"] == 1 and int(m.n[1]) == 2 and list(m.ids[1, :2]) == [2, 3] and list(m.live[1, :2]) == [True, False]
    assert m.observers(m.entry(2)) == [0, 1] and not m.flags[2] & npk.F_OBS      # key-frame 1 is not the newest
    # not one-to-one: a prev twice, a new twice, an id on both sides -- status 1, nothing changed
    for pairs in ([(5, 1), (5, 2)], [(5, 1), (4, 1)], [(5, 1), (1, 2)]):
        m = _small()
        snap = nm.snapshot(m)
        assert not nm.check_pairs(pairs)
        out = nm.merge(m, pairs, None)
        assert out["status"] == 1 and out["applied"] == 0 and nm.snapshot(m) == snap
    assert nm.check_pairs([(5, 1), (4, 2), (3, 3)])
