"""CPU: the model of slam_kfmap_triangulate_temporal (tests/np_kfmap_tri.py) on the sequences of tests/kfmap_tri_scripts.py.

  * every sequence finds a scene that passes the guard (gate quantities 1e-6 away from their thresholds, the rotated bearing's z 0.1 away from zero)
    within three seeds, and holds the cases it is there for;
  * on the sequences where nothing is forgotten the model equals, after every step, a literal dict-and-set restatement of triangulate_temporal!,
    update_mappoint! and remove_mappoint_obs! on tests/tracked_ba.py's unbounded Record: decisions, observers, masks and flags array_equal, positions
    equal (both are numpy);
  * four mutants of the model are each rejected by at least one sequence;
  * the two states of a 2-D point the seams cannot produce (a tombstone in the first observer's slab under a set bit; the first observer's bit cleared
    while its key-frame stays) are set by hand on model and record, and both give the stated decision;
  * kfm_first_observer (csrc/kfmap_ring.hpp) as a stand-alone program (tests/c_host/kfmap_tri_check.cpp), built plain and with
    -fsanitize=address,undefined (the program alone; nothing is loaded into Python), against the numpy rule: all masks of R = 4 with every tag
    pattern, random masks at R = 64."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_tri_scripts as ts  # noqa: E402
import np_kfmap as npk  # noqa: E402
import np_kfmap_tri as nt  # noqa: E402
import tracked_ba as tb  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "kfmap_tri_check.cpp")
INC = os.path.join(ROOT, "slam.jl_amd", "csrc")
FLAGS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def test_the_entry_point_is_declared():
    from slam_jl_amd import _lib
    assert "slam_kfmap_triangulate_temporal" in _lib.SIGNATURES, "slam_kfmap_triangulate_temporal: the model has no entry point to describe"


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driven():
    """every sequence, driven once on the model alone: {name: run}"""
    out = {}
    for name in ts.SEQUENCES:
        run, fn = ts.make(name)
        fn(run)
        out[name] = run
    return out


def _count(run, code):
    return sum(c["code"] == code for c in run.met)


def test_every_sequence_finds_a_guarded_scene_and_holds_its_cases(driven):
    for name, run in driven.items():
        assert run.seed < ts.MAX_SEEDS and ts.scene_ok(run) and run.met, name
        assert _count(run, nt.ACCEPTED) >= 5 and _count(run, nt.REMOVED) >= 2 and _count(run, nt.FEW) >= 5, (name, [_count(run, c) for c in range(1, 6)])
    # gates that fail above the parallax bar (removed) and below it (accepted as they are)
    plain = driven["plain"]
    assert any(c["code"] == nt.ACCEPTED and c["fail"] for c in plain.met) and any(c["code"] == nt.REMOVED for c in plain.met)
    # 1: at key-frame 0 every candidate has one observer, at key-frame 1 the newborn ones have (SELF cannot occur: the newest id is the largest)
    assert _count(plain, nt.SELF) == 0 and all(c["code"] == nt.FEW for c in plain.met[:sum(len(t[0][0]) for t in plain.tracks)])
    # 2 / 3: key-frame 0 is gone (removed / its slot reused) and the observer is 1 -- for points key-frame 0 had observed
    for name, last in (("withheld", 2), ("ring", 4)):
        run = driven[name]
        assert all(m.slot(0) is None for m in run.m)
        paired = [c for c in run.met if c["code"] in (nt.ACCEPTED, nt.REMOVED)]
        born1 = [run.tracks[s][1][1] for s in range(run.S)]
        assert any(c["observer"] == 1 and c["id"] < min(born1) for c in paired), name
        assert all(c["observer"] >= 1 for c in paired), name
    # 5: a point rejected at key-frame 1 and seen again: the pair skips key-frame 1
    tomb = driven["tombstones"]
    assert any(c["observer"] == 0 and c["code"] in (nt.ACCEPTED, nt.REMOVED) and 1 not in tomb.m[0].observers(c["id"] % tomb.mcap) for c in tomb.last[0]["cand"])
    # 6: orphans and dead points in the newest slab
    table = driven["table"]
    orphans = dead = 0
    for m in table.m:
        r0 = m.cur % m.R
        for i in range(int(m.n[r0])):
            e = int(m.ids[r0, i]) % m.mcap
            orphans += bool(m.live[r0, i]) and m.ptag[e] != m.ids[r0, i]
            dead += bool(m.live[r0, i]) and m.ptag[e] == m.ids[r0, i] and bool(m.flags[e] & npk.F_DEAD)
    assert orphans >= 1, "table: no orphan in a newest slab"
    assert any(m.flags[e] & npk.F_DEAD for m in table.m for e in range(m.mcap)), "table: no dead point"
    # 7: the unselected stream was not acted on
    assert driven["selection"].last[1] is None and driven["selection"].last[0] is not None
    # 8: the newest slabs span two workgroups, with candidates behind observation 256
    wide = driven["wide"]
    assert all(257 <= int(m.n[m.cur % m.R]) <= 300 for m in wide.m)
    assert all(any(int(np.searchsorted(m.ids[m.cur % m.R, :int(m.n[m.cur % m.R])], c["id"])) >= 256 and c["code"] in (nt.ACCEPTED, nt.REMOVED) for c in r["cand"])
               for m, r in zip(wide.m, wide.last))
    # 9: a removed observation dropped the row keyed k and the point stays described
    rows = driven["rows"]
    hit = 0
    for s, r in enumerate(rows.last):
        for c in r["cand"]:
            if c["code"] == nt.REMOVED:
                e = c["id"] % rows.mcap
                assert rows.m[s].cur not in rows.D[s]["krows"][e]
                hit += bool(rows.D[s]["has"][e]) and len(rows.D[s]["krows"][e]) >= 1
    assert hit >= 1
    # 11: a candidate whose list index differs from its slab index was triangulated into the list
    merged = driven["merged"]
    shifted = 0
    for s, r in enumerate(merged.last):
        m, lst = merged.m[s], merged.lists[s]
        r0 = m.cur % m.R
        for c in r["cand"]:
            if c["code"] == nt.ACCEPTED:
                i, l = int(np.searchsorted(m.ids[r0, :int(m.n[r0])], c["id"])), np.flatnonzero(lst["ids"] == c["id"])
                assert len(l) == 1 and lst["is_3d"][l[0]] and np.array_equal(lst["xyz"][l[0]], c["xyz"])
                shifted += int(l[0]) != i
    assert shifted >= 1 and all(len(p) >= 1 for p in merged.pairs)


def test_refined_poses_move_the_world_points():
    """4: a condition on the scene, not a tolerance on the code -- the points computed with the refined pose differ from those computed with the
    unrefined pose by more than 1e-6"""
    a, fn = ts.make("refined")
    fn(a)
    b, _ = ts.make("refined")
    b.solution = lambda s, win, outliers=None: (np.asarray(win["theta"]).copy(), np.zeros(len(win["obs_kf"]), dtype=bool))      # the unrefined twin
    fn(b)
    n = 0
    for ra, rb in zip(a.last, b.last):
        pa, pb = {c["id"]: c["xyz"] for c in ra["cand"] if c["code"] == nt.ACCEPTED}, {c["id"]: c["xyz"] for c in rb["cand"] if c["code"] == nt.ACCEPTED}
        for i in set(pa) & set(pb):
            assert np.abs(pa[i] - pb[i]).max() > 1e-6, i
            n += 1
    assert n >= 10


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------------------
class Both(ts.TriRun):
    """TriRun with a tracked_ba.Record beside every model, given the same steps; same() holds them equal"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.rec = [tb.Record(ts.CAM, None, self.minc, 0.0) for _ in range(self.S)]
        for m in self.m:
            m.theta_fn = tb.theta_of
        self.logs = None

    def add(self, mask=None):
        took = super().add(mask)
        for s, f in took.items():
            tb.add_keyframe(self.rec[s], self.nkf[s] - 1, f["Tcw"], dict(ids=f["ids"], yx=f["yx"], is_3d=f["is_3d"], xyz=f["xyz"]))
        return took

    def tri(self, mutant=None, with_list=None):
        out = super().tri(mutant, with_list)
        self.logs = [nt.restated(self.rec[s], ts.CAM, ts.MAX_ERROR, ts.MIN_DEPTH, ts.MIN_PARALLAX) if self.sel[s] else None for s in range(self.S)]
        return out

    def gather(self):
        wins = super().gather()
        self.rwins = {s: tb.gather(self.rec[s]) for s in range(self.S) if self.sel[s]}
        assert sorted(wins) == sorted(s for s, w in self.rwins.items() if w is not None)
        for s, w in wins.items():
            for k in ("theta", "pixels", "obs_kf", "obs_kp", "obs_in_covmap", "points_remap", "poses_remap"):
                assert np.array_equal(np.asarray(w[k]), np.asarray(self.rwins[s][k])), (s, k)
        return wins

    def update(self, wins, sols):
        super().update(wins, sols)
        for s in wins:
            tb.update(self.rec[s], self.rwins[s], *sols[s])

    def same(self):
        for s, (rec, m) in enumerate(zip(self.rec, self.m)):
            assert sorted(int(t) for t in m.tag if t >= 0) == sorted(rec.kfs)
            for kfid, kf in rec.kfs.items():
                mk = m.keyframe(kfid)
                assert np.array_equal(mk["theta"], kf.theta), (s, kfid)
                assert {int(i): (float(p[0]), float(p[1])) for i, p, l in zip(mk["ids"], mk["upx"], mk["live"]) if l} == kf.px, (s, kfid)
            pts = m.points()
            assert list(pts["ids"]) == sorted(rec.mps), s
            for j, i in enumerate(pts["ids"]):
                mp = rec.mps[int(i)]
                assert pts["observers"][j] == tuple(sorted(mp.obs)) and np.array_equal(pts["xyz"][j], mp.xyz), (s, i)          # masks, positions
                assert (pts["is_3d"][j], pts["observed"][j], pts["ba"][j]) == (mp.is_3d, mp.observed, mp.ba), (s, i)            # flags
            if self.logs is not None and self.logs[s] is not None and self.last is not None:
                got = [(c["id"], c["code"], c["observer"]) for c in self.last[s]["cand"]]
                assert got == self.logs[s], s                                                                                     # decisions, observers


@pytest.mark.parametrize("name", ts.UNBOUNDED)
def test_model_equals_the_restatement_after_every_step(name):
    run, fn = ts.make(name, cls=Both)
    steps = []
    run.on_step = lambda step: (run.same(), steps.append(step))
    fn(run)
    assert len(steps) >= 4 and any(log for log in run.logs if log)


@pytest.mark.parametrize("mutant", nt.MUTANTS)
def test_mutants_are_rejected(mutant):
    rejected = []
    for name in ts.UNBOUNDED:
        run, fn = ts.make(name, cls=Both)
        tri = run.tri
        run.tri = lambda m=None, with_list=None, tri=tri: tri(mutant, with_list)
        run.on_step = lambda step: run.same()
        try:
            fn(run)
        except AssertionError:
            rejected.append(name)
    assert rejected, "no sequence rejects the mutant " + mutant


def test_the_states_the_seams_cannot_produce():
    """Sequence 5 as the issue words it.  A window holds 3-D points only, so update never clears an observer bit of a 2-D point, and every seam that
    writes a tombstone clears the bit with it: both states are set by hand.  (a) a tombstone in the first observer's slab, the bit still set: ABSENT,
    nothing changes.  (b) the first observer's bit cleared, its key-frame still in the ring: the next observer is taken."""
    run, _ = ts.make("tombstones", cls=Both)
    for _ in range(3):
        run.add()                                                # key-frames 0, 1, 2, triangulation withheld: observers 0, 1, 2
    m, rec = run.m[0], run.rec[0]
    old = [int(i) for i in m.ids[2 % m.R, :int(m.n[2 % m.R])] if m.observers(int(i) % m.mcap) == [0, 1, 2]]
    a, b = old[0], old[1]
    m.live[0, m.find_live(0, a)] = False; rec.kfs[0].px.pop(a)                                    # (a)
    m.mask[b % m.mcap] &= ~1; rec.mps[b].obs.discard(0)                                          # (b)
    run.tri()
    run.same()
    by = {c["id"]: c for c in run.last[0]["cand"]}
    assert (by[a]["code"], by[a]["observer"]) == (nt.ABSENT, 0) and not m.flags[a % m.mcap] & npk.F_3D and m.observers(a % m.mcap) == [0, 1, 2]
    assert by[b]["code"] in (nt.ACCEPTED, nt.REMOVED) and by[b]["observer"] == 1


# ---- kfm_first_observer ------------------------------------------------------------------------------------------------------------------------------------
def np_first_observer(mask, tag, R):
    """the numpy rule: among the bits below R whose slot has a tag, the slot of the smallest tag; fewer than two: -1"""
    bits = np.array([b for b in range(64) if mask >> b & 1 and b < R and tag[b] != 0], dtype=np.int64)
    if len(bits) < 2:
        return -1
    return int(bits[np.argmin(np.asarray(tag)[bits])])


def cases():
    out = []
    for tag in itertools.chain(itertools.permutations((1, 2, 3, 4)), itertools.permutations((0, 5, 6, 7)), itertools.permutations((0, 0, 9, 3)),
                               [(0, 0, 0, 0), (0, 0, 0, 2), (7, 8, 9, 10), (10, 9, 8, 7)]):
        for mask in range(16):
            out.append((4, mask, tuple(tag)))
            out.append((4, mask | (0xABCD << 4), tuple(tag)))    # bits at and above R mean nothing
    rng = np.random.default_rng(64)
    for _ in range(400):
        tag = rng.permutation(np.arange(1, 65) + int(rng.integers(0, 1000)))
        tag[rng.random(64) < rng.random()] = 0
        mask = int(rng.integers(0, 1 << 63)) << 1 | int(rng.integers(0, 2))
        if rng.random() < 0.3:
            mask &= int(rng.integers(0, 1 << 63))
        out.append((64, mask & 0xFFFFFFFFFFFFFFFF, tuple(int(t) for t in tag)))
    return out


@pytest.mark.parametrize("flags", sorted(FLAGS))
def test_first_observer_equals_the_numpy_rule(flags, tmp_path):
    exe = str(tmp_path / "kfmap_tri_check")
    cxx = os.environ.get("CXX", "c++")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC] + FLAGS[flags] + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    cs = cases()
    r = subprocess.run([exe], input="".join("%d %d %s\n" % (R, mask, " ".join(str(t) for t in tag)) for R, mask, tag in cs), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = [int(v) for v in r.stdout.split()]
    want = [np_first_observer(mask, tag, R) for R, mask, tag in cs]
    assert got == want
    assert {-1, 0, 1, 2, 3} <= set(want[:2000]) and max(want) >= 40
