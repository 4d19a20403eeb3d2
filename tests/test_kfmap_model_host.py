"""CPU: the bounded key-frame map model (tests/np_kfmap.py, the layout of csrc/kfmap.hpp) against tests/tracked_ba.py's Record on scripted
key-frame sequences (tests/kfmap_scripts.py).

Where nothing is forgotten (key-frames < R, ids < mcap) every gathered array and every snapshot after update is array_equal, and the scenarios
are shown to contain the cases that make that equality mean something.  Where the ring or the table wraps, the model must differ from the
unbounded record ONLY by what was forgotten: the record is given exactly those forgettings as explicit operations (the key-frame that left the
ring is removed as remove_keyframe! does, the point whose entry a newer id took is dropped, an id that found its entry taken is not
recorded) and then equals the model again, window for window."""
import numpy as np
import pytest

import kfmap_scripts as scr
import np_kfmap as km
import tracked_ba as tb


class LogRecord(tb.Record):
    """Record that notes which co-key-frames a gather walks (ids_3d is called for exactly those)"""
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.walked = []

    def ids_3d(self, kfid):
        self.walked.append(kfid)
        return super().ids_3d(kfid)


def _orc_undistort(cam, dist, yx):
    from oracle import oracle as orc
    return np.array([orc.undistort_point(cam, dist, p) for p in yx]).reshape(-1, 2)


def _same_window(wr, wm):
    for k in ("theta", "theta_const", "pixels", "poses_ids", "points_ids", "obs_kf", "obs_kp", "obs_in_covmap", "poses_remap", "points_remap"):
        assert np.array_equal(np.asarray(wr[k]), np.asarray(wm[k])), k
    assert wr["kfid"] == wm["kfid"] and set(wr["bad"]) == set(wm["bad"])


def _same_state(rec, m, with_pixels=True):
    for kfid, kf in rec.kfs.items():
        mk = m.keyframe(kfid)
        assert mk is not None and np.array_equal(mk["theta"], kf.theta), kfid
        if with_pixels:
            px = {int(i): (float(p[0]), float(p[1])) for i, p, l in zip(mk["ids"], mk["upx"], mk["live"]) if l}
            assert px == kf.px, kfid
    assert sorted(int(t) for t in m.tag if t >= 0) == sorted(rec.kfs)
    pts = m.points()
    assert list(pts["ids"]) == sorted(rec.mps)
    for j, i in enumerate(pts["ids"]):
        mp = rec.mps[int(i)]
        assert np.array_equal(pts["xyz"][j], mp.xyz) and pts["observers"][j] == tuple(sorted(mp.obs)), i
        assert (pts["is_3d"][j], pts["observed"][j], pts["ba"][j]) == (mp.is_3d, mp.observed, mp.ba), i


def _run(name, bounded):
    """Drive scenario `name` through both models; yields per stream and key-frame (rec, m, wr, wm, walked, n_cov) after the gather, and checks
    the states after add_keyframe and after update.  bounded: give the record the ring's and the table's forgettings."""
    sc, streams = scr.scenario(name)
    R, mcap = sc["R"], sc["mcap"]
    for s, frames in enumerate(streams):
        dist = sc["dists"][s]
        rec = LogRecord(scr.CAM, dist, sc["minc"][s], 0.0)
        m = km.Map(scr.CAP, R, mcap, scr.CAM, dist, sc["minc"][s], theta_fn=tb.theta_of, undistort_fn=_orc_undistort)
        owner = {}
        for k, f in enumerate(frames):
            lst = dict(ids=f["ids"], yx=f["yx"], is_3d=f["is_3d"], xyz=f["xyz"])
            lst_r = lst
            if bounded:
                if k - R in rec.kfs:                             # remove_keyframe! (map_manager.jl:184-209)
                    for kp in rec.kfs[k - R].px:
                        if kp in rec.mps:
                            rec.mps[kp].obs.discard(k - R)
                    del rec.kfs[k - R]
                for i in (int(i) for i in f["ids"]):             # the table: the largest id owns an entry, the point it replaces is gone
                    e = i % mcap
                    if i in rec.gone and owner.get(e) == i:
                        continue
                    if owner.get(e, -1) < i:
                        if e in owner:
                            rec.mps.pop(owner[e], None)
                        owner[e] = i
                keep = np.array([owner.get(int(i) % mcap) == int(i) for i in f["ids"]], dtype=bool)
                lst_r = {a: v[keep] for a, v in lst.items()}
            else:
                assert k < R and (len(f["ids"]) == 0 or f["ids"].max() < mcap), "the plain scenario forgets nothing"
            tb.add_keyframe(rec, k, f["Tcw"], lst_r)
            km.add_keyframe(m, k, f["Tcw"], lst)
            _same_state(rec, m, with_pixels=not bounded)
            n_cov = len(tb.covisibility(rec, k)) + 1
            rec.walked = []
            wr, wm = tb.gather(rec), km.gather(m)
            walked = list(rec.walked)
            if wr is None or len(wr["poses_ids"]) == 0:
                assert wm is None
            else:
                _same_window(wr, wm)
            yield s, k, rec, m, wr, wm, walked, n_cov
            if wr is None:
                continue
            ol, th = scr.outlier_pattern(sc["seeds"][s], wr), scr.refined(sc["seeds"][s], wr)
            tb.update(rec, wr, th, ol)
            if wm is not None:
                km.update(m, wm, th, ol)
            _same_state(rec, m, with_pixels=not bounded)
            assert m.gone() == tuple(sorted(i for i in rec.gone if not bounded or owner.get(i % mcap) == i))


def test_plain_scenario_equals_the_record_and_contains_the_cases():
    seen = dict.fromkeys(("single_free", "const_only", "const_not0", "truncated", "low_skipped", "low_walked", "outside_covmap", "below_min",
                          "first_empty", "demoted", "out_in_covmap", "out_not_covmap", "out_own_kf", "point_removed"), 0)
    sc = scr.SCENARIOS["plain"]
    flagged, last = [], {}
    for s, k, rec, m, wr, wm, walked, n_cov in _run("plain", bounded=False):
        if wr is None:
            seen["below_min"] += 1
            continue
        if len(wr["poses_ids"]) == 0:
            seen["first_empty"] += k == 0
            continue
        st = tb.structure(wr)
        seen["single_free"] += st["single_free"] > 0; seen["const_only"] += st["const_only"] > 0; seen["const_not0"] += st["const_not0"] > 0
        seen["truncated"] += n_cov > tb.N_COVISIBLE
        minc = sc["minc"][s]
        for co, score in wr["covmap"].items():
            if 0 < score < minc and co != 0:
                seen["low_walked"] += co in walked
                seen["low_skipped"] += co not in walked and rec.nb_3d(co) > 0
        seen["outside_covmap"] += bool((~wr["obs_in_covmap"]).any())
        seen["demoted"] += len(wr["bad"]) > 0
        ol = scr.outlier_pattern(sc["seeds"][s], wr)
        seen["out_in_covmap"] += bool((ol & wr["obs_in_covmap"]).any()); seen["out_not_covmap"] += bool((ol & ~wr["obs_in_covmap"]).any())
        seen["out_own_kf"] += bool((ol & (wr["obs_kf"] == k)).any())
        flagged += [(s, int(kp)) for kp in np.unique(wr["obs_kp"]) if ol[wr["obs_kp"] == kp].all()]
        last[s] = (rec, m)
    # a point whose every observation was flagged is removed (where the flagged observations lay inside the covisibility map)
    seen["point_removed"] = sum(1 for s, kp in flagged if kp not in last[s][0].mps and last[s][1].entry(kp) is None)
    missing = [c for c, n in seen.items() if n == 0]
    assert not missing, (missing, seen)


@pytest.mark.parametrize("name", ["ring", "table"])
def test_wrapped_scenarios_differ_only_by_what_was_forgotten(name):
    sc = scr.SCENARIOS[name]
    n_win, forgot_kf, forgot_pt = 0, 0, 0
    for s, k, rec, m, wr, wm, walked, n_cov in _run(name, bounded=True):
        n_win += wm is not None
        forgot_kf += k >= sc["R"]
        forgot_pt += len(m.points()["ids"]) > 0 and k == len(sc["sizes"][s]) - 1 and any(m.ptag[e] >= sc["mcap"] for e in range(sc["mcap"]))
    assert n_win >= 6
    assert forgot_kf > 0 if name == "ring" else forgot_pt > 0
