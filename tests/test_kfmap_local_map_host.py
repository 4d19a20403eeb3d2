"""CPU: the model of slam_kfmap_local_map_match (tests/np_kfmap_local_map.py) on the scripted scenes of tests/kfmap_lmm_scripts.py.

  * model against restatement: where nothing is forgotten (a ring and a table larger than the sequence, no bundle adjustment) the model's local map
    equals a plain dict-and-set restatement of update_frame_covisibility! (src/map_manager.jl:302-343) on tests/tracked_ba.py's unbounded Record;
  * the scenes the GPU tests run (S = 3, cap 64, R = 4, mcap = 128, a 70 x 105 image with cell 35, 8 key-frames) reach what they are meant to reach:
    margin >= 1e-9, at least one pair per matching stream and call, the ring and the table wrap, an entry with a descriptor changes owner, projections
    fall in corner cells and outside the image, ties occur;
  * mutants: each of four broken rules changes the result on at least one scene.
The model describes entry points of the library: every test here first asserts that they exist."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_lmm_scripts as ls  # noqa: E402
import np_kfmap as npk  # noqa: E402
import np_local_map as nlm  # noqa: E402

ENTRY_POINTS = ("slam_kfmap_enable_descriptors", "slam_kfmap_add_descriptors", "slam_kfmap_local_map_match")


@pytest.fixture(autouse=True)
def entry_points():
    import slam_jl_amd
    from slam_jl_amd import _lib
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, f"{name}: the model has no entry point to describe"
    for name in ("enable_descriptors", "add_descriptors", "local_map_match"):
        assert hasattr(slam_jl_amd.KeyframeMap, name)


def _same(a, b):
    return a["status"] == b["status"] and all(np.array_equal(a[k], b[k]) for k in ("lm_ids", "pairs", "dist"))


def _gpu_sequence(mutants=()):
    """the sequence tests/test_gpu_kfmap_local_map.py runs -> [(key-frame, stream, result, {mutant: result})] of the streams acted on"""
    frames, descs = ls.scenes()
    run = ls.ModelRun(frames, descs)
    out = []
    for k in range(ls.N_KF):
        run.add(ls.LAST_MASK if k == ls.N_KF - 1 else None)
        r = run.match()
        alt = {mu: run.match(mutant=mu) for mu in mutants}
        out += [(k, s, r[s], {mu: alt[mu][s] for mu in mutants}) for s in range(ls.S) if run.sel[s]]
        if k in ls.BA_AT:
            run.ba()
    return run, out


def _restated_local_map(rec, described, kfid):
    """update_frame_covisibility! (map_manager.jl:302-343) on the unbounded record, dicts and sets only; the descriptor gate of mapper.jl:341"""
    covisible_keyframes = {}
    for kpid in rec.kfs[kfid].px:                                               # :309
        mp = rec.mps.get(kpid)
        if mp is None:                                                          # :310-314
            continue
        for o in mp.obs:                                                        # :318-325
            if o != kfid:
                covisible_keyframes[o] = covisible_keyframes.get(o, 0) + 1
    local_map_ids = set()
    for o in covisible_keyframes:                                               # :333
        if o not in rec.kfs:                                                    # :334-337
            continue
        for kpid in rec.ids_3d(o):                                              # :340 get_3d_keypoints
            if kpid not in rec.kfs[kfid].px and kpid in described:              # :341
                local_map_ids.add(kpid)
    return sorted(local_map_ids)


def test_model_local_map_equals_the_restatement_where_nothing_is_forgotten():
    import tracked_ba as tb
    import np_kfmap_local_map as nl
    frames, descs = ls.scenes()
    n_points = 0
    for s in range(ls.S):
        m = npk.Map(ls.CAP, 16, 1024, ls.CAM10[:4])
        D = nl.new_descriptors(m)
        rec, described = tb.Record(ls.CAM10[:4]), set()
        for k, (f, d) in enumerate(zip(frames[s], descs[s])):
            nl.add_keyframe(m, D, k, f["Tcw"], f); nl.add_descriptors(m, D, d[0], d[1])
            tb.add_keyframe(rec, k, f["Tcw"], f); described |= set(range(int(d[0]), int(d[0]) + len(d[1])))
            want = _restated_local_map(rec, described, k)
            cov = nl.covisible_slots(m)
            assert nl.local_map_ids(m, D, cov) == want, (s, k)
            assert sorted(int(m.tag[b]) for b in cov) == sorted(tb.covisibility(rec, k)), (s, k)
            r = nl.local_map_match(m, D, ls.CAM10, ls.CELL, ls.PARAMS)
            assert list(r["lm_ids"]) == (want if r["status"] == 0 else []), (s, k)
            n_points += len(want)
    assert n_points > 300


def test_the_gpu_scenes_reach_their_edges():
    run, seq = _gpu_sequence()
    matched = [(k, s, r) for k, s, r, _ in seq if r["status"] == 0]
    assert {s for _, s, _ in matched} == set(range(ls.S))
    for k, s, r in matched:
        assert r["margin"] >= 1e-9, (k, s, r["margin"])
        assert len(r["pairs"]) >= 1, (k, s)
        assert np.all(np.diff(r["pairs"][:, 0]) > 0) and np.all(np.diff(r["lm_ids"]) > 0)
    assert any(r["status"] == 1 for _, _, r, _ in seq)
    count = {key: sum(r["count"][key] for _, _, r in matched) for key in ("overlap", "average", "ties_forward", "ties_reverse", "gated", "contested")}
    assert all(v > 0 for v in count.values()), count
    # the ring and the table wrap; an entry whose point had a descriptor changes owner
    assert all(run.nkf[s] > ls.R for s in range(ls.S))
    assert any(int(run.frames[s][run.nkf[s] - 1]["ids"].max()) >= ls.MCAP for s in range(ls.S)) and run.replaced >= 5
    # projections in the four corner cells of the 2 x 3 grid, and local-map points whose projection leaves the image (gated above)
    cells = set()
    for _, _, r in matched:
        for p in r["proj_yx"][~np.isnan(r["proj_yx"][:, 0])]:
            cells.add(nlm.to_cartesian(p, ls.CELL))
    assert {(1, 1), (1, 3), (2, 1), (2, 3)} <= cells
    sizes = {len(f["ids"]) for s in range(ls.S) for f in run.frames[s]}
    assert {0, 1, 63, 64} <= sizes


def test_each_mutant_changes_a_result():
    mutants = ("own", "descending", "lt", "dead")
    _, seq = _gpu_sequence(mutants)
    for mu in mutants:
        changed = [(k, s) for k, s, r, alt in seq if not _same(r, alt[mu])]
        assert changed, f"no scene tells the mutant `{mu}` from the model"
    # the order rules decide PAIRS, not only the staged order
    for mu in ("descending", "lt", "dead"):
        assert any(not (np.array_equal(r["pairs"], alt[mu]["pairs"]) and np.array_equal(r["dist"], alt[mu]["dist"])) for _, _, r, alt in seq), mu


def test_descriptors_follow_the_tables_ownership_rule():
    import np_kfmap_local_map as nl
    m = npk.Map(8, 4, 4, ls.CAM10[:4])
    D = nl.new_descriptors(m)
    lst = lambda ids: dict(ids=np.array(ids, dtype=np.int64), yx=np.full((len(ids), 2), 5.0), is_3d=np.ones(len(ids), dtype=bool), xyz=np.ones((len(ids), 3)))
    rows = lambda ids: np.array([[i + 1, 0, 0, 0] for i in ids], dtype=np.uint64)
    nl.add_keyframe(m, D, 0, np.eye(4), lst([0, 1, 2])); nl.add_descriptors(m, D, 0, rows([0, 1, 2]))
    assert list(D["has"]) == [True, True, True, False] and int(D["rows"][1, 0]) == 2
    nl.add_keyframe(m, D, 1, np.eye(4), lst([1, 2, 5]))                          # id 5 claims entry 1: the descriptor of id 1 goes with its entry
    assert list(D["has"]) == [True, False, True, False]
    nl.add_descriptors(m, D, 5, rows([5]))
    assert list(D["has"]) == [True, True, True, False] and int(D["rows"][1, 0]) == 6
    nl.add_descriptors(m, D, 1, rows([1]))                                       # a row for an id that does not own its entry is dropped
    assert int(D["rows"][1, 0]) == 6
