"""CPU: the model of slam_kfmap_local_map_match with the local-map history (tests/np_kfmap_local_map_history.py) on the sequences of
tests/kfmap_history_scripts.py.

  * model against restatement: where nothing is forgotten (a ring and a table larger than the sequence, no bundle adjustment; key-frame k - 6 leaves
    by remove_keyframe! as key-frame k arrives, or every key-frame would stay covisible and the chain would have nothing to add) the staged local maps,
    the pairs and the distances equal those of a literal dict-and-set restatement of update_frame_covisibility! + match_local_map!
    (src/map_manager.jl:302-355, src/mapper.jl:269-286) on tests/tracked_ba.py's unbounded Record, which keeps a Set per key-frame, stores RAW ids and
    gates at match time -- with and without the merges applied;
  * the main scene (S 3, cap 64, R 6, mcap 128, 12 key-frames, merges applied, an update behind key-frames 3 and 4) reaches what it is there for: on
    every stream a pair whose local-map id lies outside C(K), purged ids, re-used ring slots, margins >= 1e-9;
  * a second match for the same key-frame runs both branches of the replace-or-union rule with a non-empty P;
  * each of four mutants changes a result; two calls on an unchanged map give the same results and the same stored sets.
The model describes entry points of the library: every test here first asserts that they exist."""
import copy
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_history_scripts as hs  # noqa: E402
import kfmap_lmm_scripts as ls  # noqa: E402
import np_kfmap as npk  # noqa: E402
import np_kfmap_filter as npf  # noqa: E402
import np_kfmap_local_map as nl  # noqa: E402
import np_kfmap_local_map_history as nh  # noqa: E402
import np_kfmap_merge as nm  # noqa: E402
import np_local_map as nlm  # noqa: E402

ENTRY_POINTS = ("slam_kfmap_enable_local_map_history", "slam_kfmap_download_local_map_ids")


@pytest.fixture(autouse=True)
def entry_points():
    import slam_jl_amd
    from slam_jl_amd import _lib
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, f"{name}: the model has no entry point to describe"
    for name in ("enable_local_map_history", "local_map_ids"):
        assert hasattr(slam_jl_amd.KeyframeMap, name)


def _same(a, b):
    return a["status"] == b["status"] and all(np.array_equal(a[k], b[k]) for k in ("lm_ids", "pairs", "dist"))


# ---- the literal restatement -----------------------------------------------------------------------------------------------------------------------------
def _restated(rec, local_map_ids, described, rows, kfid, max_nb_mappoints=math.inf):
    """update_frame_covisibility! then match_local_map! for key-frame kfid of the record; local_map_ids: {kfid: set}, the frames' fields
    -> (staged ids ascending, the match's out or None)"""
    frame = rec.kfs[kfid]
    covisible_keyframes, new_ids = {}, set()
    for kpid in frame.px:                                                       # map_manager.jl:309-326
        mp = rec.mps.get(kpid)
        if mp is None:
            continue
        for o in mp.obs:
            if o != kfid:
                covisible_keyframes[o] = covisible_keyframes.get(o, 0) + 1
    for o in sorted(covisible_keyframes):                                       # :333-343 -- raw ids: no descriptor gate here
        if o not in rec.kfs:
            covisible_keyframes.pop(o)
            continue
        for kpid in rec.ids_3d(o):
            if kpid not in frame.px:
                new_ids.add(kpid)
    mine = local_map_ids.setdefault(kfid, set())
    if len(new_ids) > 0.5 * len(mine):                                          # :350-354
        mine = local_map_ids[kfid] = new_ids
    else:
        mine |= new_ids
    if len(mine) < max_nb_mappoints and covisible_keyframes:                    # mapper.jl:274-286 (an empty covisibility map: nothing to take)
        co = sorted(covisible_keyframes)[0]
        if co in rec.kfs:
            mine |= local_map_ids.get(co, set())
    staged = []
    for kpid in sorted(mine):                                                   # do_local_map_matching's gates, mapper.jl:337-341
        if kpid in frame.px:
            continue
        mp = rec.mps.get(kpid)
        if mp is None or not mp.is_3d or kpid not in described:
            continue
        staged.append(kpid)
    order = sorted(rec.kfs)
    row = {k: j for j, k in enumerate(order)}
    kp_ids = [i for i in sorted(frame.px) if i in rec.mps and i in described]
    if not staged or not kp_ids:
        return staged, kp_ids, None
    keypoints = [{"pixel": tuple(frame.px[i]), "descriptors": rows[i].reshape(1, 4),
                  "observers": [(row[o], tuple(rec.kfs[o].px[i])) for o in sorted(rec.mps[i].obs) if o in rec.kfs and i in rec.kfs[o].px]} for i in kp_ids]
    local_map = [{"position": rec.mps[i].xyz, "descriptors": rows[i].reshape(1, 4), "observers": [row[o] for o in sorted(rec.mps[i].obs) if o in rec.kfs]} for i in staged]
    fr = {"Tcw": nl.tcw_of(frame.theta), "cam": list(ls.CAM10), "cell_size": ls.CELL, "nb_3d_kpts": rec.nb_3d(kfid)}
    out = nlm.do_local_map_matching(fr, keypoints, np.array([nl.tcw_of(rec.kfs[k].theta) for k in order]), local_map, ls.PARAMS)
    return staged, kp_ids, out


@pytest.mark.parametrize("merges", (False, True))
def test_model_equals_the_literal_restatement_where_nothing_is_forgotten(merges):
    import tracked_ba as tb
    frames, descs = ls.scenes(sizes=hs.SIZES, window=hs.WINDOW)
    n_chain = n_pairs = 0
    for s in range(hs.S):
        assert max(int(f["ids"].max()) for f in frames[s] if len(f["ids"])) < 2048
        m = npk.Map(hs.CAP, 16, 2048, ls.CAM10[:4])
        D, H = nl.new_descriptors(m), nh.History(16)
        rec, described, rows, sets = tb.Record(ls.CAM10[:4]), set(), {}, {}
        for k, (f, d) in enumerate(zip(frames[s], descs[s])):
            if k >= hs.R:                                                       # remove_keyframe! of the key-frame the main scene's ring would forget here
                npf.remove_keyframe(m, k - hs.R); npf.remove_keyframe_record(rec, k - hs.R)
            nl.add_keyframe(m, D, k, f["Tcw"], f); nl.add_descriptors(m, D, d[0], d[1])
            tb.add_keyframe(rec, k, f["Tcw"], f)
            described |= set(range(int(d[0]), int(d[0]) + len(d[1]))); rows.update({int(d[0]) + j: r for j, r in enumerate(d[1])})
            got = nh.local_map_match(m, D, H, ls.CAM10, ls.CELL, ls.PARAMS)
            staged, kp_ids, out = _restated(rec, sets, described, rows, k)
            assert got["margin"] >= 1e-9
            if got["status"] == 0:
                assert list(got["lm_ids"]) == staged and list(got["kp_ids"]) == kp_ids, (s, k)
                took = np.flatnonzero(out["match"] >= 0)
                assert np.array_equal(got["pairs"], np.array([(kp_ids[j], staged[out["match"][j]]) for j in took], dtype=np.int64).reshape(-1, 2)), (s, k)
                assert np.array_equal(got["dist"], out["best_dist"][out["match"][took]]), (s, k)
            else:
                assert got["status"] == 1 and (not staged or not kp_ids), (s, k)
            assert set(H.sets[k % 16]) <= sets[k]                              # the model's set: the restatement's ids that passed the gates when stored
            n_chain += len(set(got["lm_ids"]) - set(got["C"])); n_pairs += len(got["pairs"])
            if merges and got["status"] == 0 and len(got["pairs"]):
                nm.merge(m, got["pairs"], None, with_list=False)
                for a, b in got["pairs"]:
                    nm.restated_merge(rec, int(a), int(b), with_list=False)
    assert n_chain >= 30 and n_pairs >= 60


# ---- the main scene ----------------------------------------------------------------------------------------------------------------------------------------
def _main_sequence(mutants=(), n_kf=hs.N_KF):
    """-> (run, [(key-frame, stream, result, {mutant: (result, stored-set snapshot)}, stored-set snapshot)])"""
    run, out = hs.HistoryRun(), []

    def on_step(kind, k, data):
        if kind == "match":
            for s in range(hs.S):
                out.append((k, s, data[s], run.H[s].snapshot()))
    hs.run_sequence(run, n_kf=n_kf, on_step=on_step)
    return run, out


def test_the_main_scene_reaches_what_it_is_there_for():
    run, seq = _main_sequence()
    outside = [0] * hs.S
    for k, s, r, _ in seq:
        assert r["margin"] >= 1e-9, (k, s, r["margin"])
        outside[s] += sum(1 for p in r["pairs"] if int(p[1]) not in set(r["C"]))
    assert min(outside) >= 1, outside                                           # on every stream a pair only the chain brings
    assert all(h.count["purged"] >= 10 and h.count["chained"] >= 3 for h in run.H), [h.count for h in run.H]
    assert all(run.nkf[s] > hs.R for s in range(hs.S))                          # ring slots are re-used
    assert all(int(run.frames[s][-1]["ids"].max()) >= hs.MCAP for s in range(hs.S))          # the table wraps
    assert max(len(x) for h in run.H for x in h.sets) < hs.MCAP


def test_history_off_is_the_parents_model():
    """the same sequence without history: np_kfmap_local_map's results, and the chain-reached pairs are absent"""
    on, off = hs.HistoryRun(), hs.HistoryRun(history=False)
    extra = 0
    for k in range(hs.N_KF):
        on.add(); off.add()
        a, b = on.match(), off.match()
        for s in range(hs.S):
            C = set(a[s]["C"])
            extra += sum(1 for p in a[s]["pairs"] if int(p[1]) not in C)
            if nm.snapshot(on.m[s]) == nm.snapshot(off.m[s]):                   # (once a chain-reached pair has been merged the two maps differ)
                assert list(b[s]["lm_ids"]) == (a[s]["C"] if b[s]["status"] == 0 else []), (k, s)
                assert not any(int(p[1]) not in C for p in b[s]["pairs"])
        on.merge(hs.pairs_of(a)); off.merge(hs.pairs_of(b))
        if k in hs.BA_AT:
            on.ba(); off.ba()
    assert extra >= 3


def _second_call(want):
    """behind key-frame TWO_CALLS_AT: remove covisible key-frames of every stream that can show the `want` branch, match again"""
    run, _ = _main_sequence(n_kf=hs.TWO_CALLS_AT + 1)
    plans = [hs.plan_second_call(run, s, want) for s in range(hs.S)]
    before = [copy.deepcopy(h.count) for h in run.H]
    for s, drop in enumerate(plans):
        for k in drop or ():
            run.remove_keyframe(s, k)
    res = run.match()
    return run, plans, before, res


def test_a_second_match_for_one_key_frame_runs_both_branches_with_a_non_empty_P():
    run, plans, before, res = _second_call("union")
    assert all(p is not None for p in plans)
    for s in range(hs.S):
        assert res[s]["branch"] == "union" and run.H[s].count["union"] == before[s]["union"] + 1
        assert 2 * len(res[s]["C"]) <= res[s]["size"] and set(res[s]["C"]) < run.H[s].sets[hs.TWO_CALLS_AT % hs.R]
    run, plans, before, res = _second_call("replace")
    assert all(p is not None for p in plans)
    for s in range(hs.S):
        assert res[s]["branch"] == "replace" and run.H[s].count["replace"] == before[s]["replace"] + 1
        assert res[s]["size"] == len(res[s]["C"])
    assert all(h.count["union"] == 0 for h in _main_sequence()[0].H)            # P is empty unless the match runs twice for a key-frame


def test_each_mutant_changes_a_result():
    changed = {mu: [] for mu in nh.MUTANTS}
    run = hs.HistoryRun()

    def try_mutants(k, max_local_of=None):
        for mu in nh.MUTANTS:
            for s in range(hs.S):
                ml = None
                if mu == "le":                                                  # the bound that step 3's size meets exactly, where the chain has something to add
                    dry = nh.local_map_match(run.m[s], run.D[s], copy.deepcopy(run.H[s]), ls.CAM10, ls.CELL, ls.PARAMS)
                    if not dry["chain"]:
                        continue
                    ml = dry["size"]
                Ha, Hb = copy.deepcopy(run.H[s]), copy.deepcopy(run.H[s])
                a = nh.local_map_match(run.m[s], run.D[s], Ha, ls.CAM10, ls.CELL, ls.PARAMS, max_local=ml)
                b = nh.local_map_match(run.m[s], run.D[s], Hb, ls.CAM10, ls.CELL, ls.PARAMS, max_local=ml, mutant=mu)
                if not _same(a, b) or Ha.snapshot() != Hb.snapshot():
                    changed[mu].append((k, s, not (np.array_equal(a["pairs"], b["pairs"]) and a["status"] == b["status"])))

    def on_step(kind, k, data):
        if kind == "add":
            try_mutants(k)
    hs.run_sequence(run, on_step=on_step)
    for want in ("union", "replace"):                                           # the rule shows only with a non-empty P
        run2, plans, _, _ = _second_call(want)
        for s in range(hs.S):
            Ha, Hb = copy.deepcopy(run2.H[s]), copy.deepcopy(run2.H[s])
            a = nh.local_map_match(run2.m[s], run2.D[s], Ha, ls.CAM10, ls.CELL, ls.PARAMS)
            b = nh.local_map_match(run2.m[s], run2.D[s], Hb, ls.CAM10, ls.CELL, ls.PARAMS, mutant="rule")
            if not _same(a, b) or Ha.snapshot() != Hb.snapshot():
                changed["rule"].append((want, s, True))
    for mu in nh.MUTANTS:
        assert changed[mu], f"no scene tells the mutant `{mu}` from the model"
    # ("newest" shows in the staged lists and the stored sets only: on these scenes the points it brings instead find no keypoint)
    for mu in ("nochain", "le"):                                                # whether the chain runs decides pairs or a status, not only the stored sets
        assert any(c[2] for c in changed[mu]), mu


def test_two_calls_on_an_unchanged_map_give_the_same_results_and_sets():
    run = hs.HistoryRun()

    def on_step(kind, k, data):
        if kind == "match":
            first = [h.snapshot() for h in run.H]
            maps = [nm.snapshot(m) for m in run.m]
            again = run.match()
            assert all(_same(a, b) for a, b in zip(data, again)), k
            assert [h.snapshot() for h in run.H] == first and [nm.snapshot(m) for m in run.m] == maps, k
    hs.run_sequence(run, on_step=on_step)
    assert sum(h.count["replace"] for h in run.H) >= 20                         # (the second calls: C > 0.5 P, L = C, the chain adds what it added)
