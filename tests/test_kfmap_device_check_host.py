"""Host: the checkers of tests/kfmap_device.py, which every tests/test_gpu_kfmap_*.py run relies on, tested themselves -- no GPU.  A stand-in device
serves the read-backs the checkers make (download_keyframe, download_points, keyframe_pixels, descriptor_rows, local_map_ids, debug_local_map,
KeypointSet.download) from a deep copy of the model, in the shapes and dtypes the Python wrappers document.  The first three key-frames of
tests/kfmap_lmm_scripts.py's scenes, seen through tests/kfmap_lens_scripts.py's lens so that the raw-pixel store has something of its own to hold,
are driven through the model twice: with descriptor rows and following lists, and with the local-map history.  The clean stand-in passes
check() and check_match(); every mutant changes ONE thing in the stand-in's copy and must make the checker raise -- a checker that skipped a key
would let its mutant through."""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_device as kd  # noqa: E402
import kfmap_lens_scripts as lz  # noqa: E402
import np_kfmap as npk  # noqa: E402
import np_kfmap_rows as nr  # noqa: E402

N_KF = 3


class StandIn:
    """a KeyframeMap and a KeypointSet in one, answering from a deep copy `r` of the run (and of the last match's results)"""

    def __init__(self, run, matched):
        self.r = SimpleNamespace(**copy.deepcopy({key: getattr(run, key) for key in ("m", "D", "H", "lists")}))
        self.matched = copy.deepcopy(matched)

    def download_keyframe(self, s, k):
        return self.r.m[s].keyframe(k)

    def download_points(self, s):
        return self.r.m[s].points()

    def keyframe_pixels(self, s, k):
        return lz.LensRun.pixels(self.r, s, k)

    def descriptor_rows(self, s):
        return nr.descriptor_rows(self.r.m[s], self.r.D[s])

    def local_map_ids(self, s, k):
        ids = self.r.H[s].ids(self.r.m[s], k)
        if ids is None:
            raise LookupError("key-frame %d is not in the ring" % k if self.r.m[s].slot(k) is None else "no local map was stored for key-frame %d" % k)
        return ids

    def debug_local_map(self, s):
        return {key: self.matched[s][key] for key in ("lm_ids", "proj_yx", "best_kp", "best_dist", "kp_ids")}

    def download(self, s):
        return dict(self.r.lists[s])

    def answers(self):
        """(status, pairs, dist) as KeyframeMap.local_map_match returns them"""
        return (np.array([w["status"] for w in self.matched], dtype=np.int32), [w["pairs"] for w in self.matched], [w["dist"] for w in self.matched])


class Host(kd.DeviceSide, lz.LensRun):
    """the models alone, with DeviceSide's checkers looking at a stand-in"""

    def __init__(self, kind, mode):
        lz.LensRun.__init__(self, kind=kind, mode=mode)
        self.has_rows, self.has_history, self.has_pixels = kind == "rows", kind == "history", True
        self.matched = None

    def step(self, k, match=True, merge=True):
        lz.LensRun.add(self)
        if match:
            self.matched = lz.LensRun.match(self)
            if merge:
                lz.LensRun.merge(self, lz.pairs_of(self.matched))

    def stand_in(self, upx_tol=0.0, proj_tol=0.0):
        """a fresh stand-in of the present state; upx_tol, proj_tol: the mode the checkers compare pixels and projections in"""
        self.km = self.ks = None
        self.km = self.ks = StandIn(self, self.matched)
        self.upx_tol, self.px_tol, self.proj_tol = upx_tol, upx_tol, proj_tol
        return self.km.r, self.km


@pytest.fixture(scope="module")
def rows_run():
    """descriptor rows, raw pixels and lists that follow; key-frames 0 .. 2, the last matched and not yet merged"""
    h = Host("rows", "follow")
    for k in range(N_KF):
        h.step(k, merge=k < N_KF - 1)
    assert sum(len(w["pairs"]) for w in h.matched) >= 1 and all(h.sel)
    return h


@pytest.fixture(scope="module")
def history_runs():
    """the local-map history: (key-frame 2 recorded and not yet matched -- no set is stored for it --, the same run behind that match)"""
    runs = []
    for matched in (False, True):
        h = Host("history", "stale")
        for k in range(N_KF):
            h.step(k, match=matched or k < N_KF - 1, merge=k < N_KF - 1)
        runs.append(h)
    before, h = runs
    assert h.H[0].ids(h.m[0], N_KF - 1) is not None and before.H[0].ids(before.m[0], N_KF - 1) is None
    return before, h


@pytest.mark.parametrize("upx_tol", (0.0, kd.PX_TOL))
def test_the_clean_stand_in_passes(rows_run, history_runs, upx_tol):
    for h in (rows_run,) + history_runs:
        r, dev = h.stand_in(upx_tol)
        h.check()
        if h.matched is not None:
            h.check_match(dev.answers(), h.matched)


def _a_point(m, n_obs=1):
    return next(e for e in range(m.mcap) if m.ptag[e] >= 0 and not m.flags[e] & npk.F_DEAD and len(m.observers(e)) >= n_obs)


def live_flipped(r):
    m = r.m[0]
    m.live[m.slot(m.cur - N_KF + 1), 0] ^= True                  # the oldest slot still in the ring


def id_changed(r):
    m = r.m[0]
    m.ids[m.slot(m.cur), 0] += 10 ** 5


def upx_moved(r):
    m = r.m[1]
    m.upx[m.slot(m.cur), 3, 1] += 1e-6                           # far above PX_TOL: caught in tolerance mode too


def slot_past_the_newest(r):
    m = r.m[2]
    assert m.tag[(m.cur + 1) % m.R] < 0
    m.tag[(m.cur + 1) % m.R] = m.cur + 1; m.n[(m.cur + 1) % m.R] = 0


def observer_missing(r):
    m = r.m[0]
    e = _a_point(m, 2)
    m.mask[e] &= ~(1 << m.slot(m.observers(e)[0]))


def gone_flipped(r):
    m = r.m[1]
    m.flags[_a_point(m)] ^= npk.F_GONE


def list_longer(r):
    r.lists[0] = {key: np.concatenate([v, v[-1:] + (1 if key == "ids" else 0)]) for key, v in r.lists[0].items()}


def raw_pixel_changed(r):
    m = r.m[2]
    m.views["raw"][m.slot(m.cur), 0, 0] += 1.0


def row_under_another_key(r):
    rows = next(k for k in r.D[0]["krows"] if k)
    key = min(rows)
    rows[key + 1000] = rows.pop(key)


SLAB_MUTANTS = (live_flipped, id_changed, upx_moved, slot_past_the_newest, observer_missing, gone_flipped, list_longer, raw_pixel_changed,
                row_under_another_key)


@pytest.mark.parametrize("upx_tol", (0.0, kd.PX_TOL))
@pytest.mark.parametrize("mutant", SLAB_MUTANTS, ids=lambda f: f.__name__)
def test_check_catches_one_changed_field(rows_run, mutant, upx_tol):
    r, dev = rows_run.stand_in(upx_tol)
    mutant(r)
    with pytest.raises(AssertionError):
        rows_run.check()


def test_check_catches_a_wrong_stored_set(history_runs):
    before, h = history_runs
    r, dev = h.stand_in()
    b = r.m[0].slot(N_KF - 1)
    assert len(r.H[0].sets[b]) >= 2
    r.H[0].sets[b].discard(min(r.H[0].sets[b]))                  # an id missing
    with pytest.raises(AssertionError):
        h.check()
    with pytest.raises(AssertionError):
        h.check_match(dev.answers(), h.matched)                  # (check_match looks at the stored sets too)
    r, dev = before.stand_in()
    r.H[1].kf[r.m[1].slot(N_KF - 1)] = N_KF - 1                  # a set where the model expects "no local map was stored"
    r.H[1].sets[r.m[1].slot(N_KF - 1)] = {int(r.m[1].ids[r.m[1].slot(N_KF - 1), 0])}
    with pytest.raises(AssertionError):
        before.check()


def pairs_int32(dev, s):
    return (dev.answers()[0], [p.astype(np.int32) for p in dev.answers()[1]], dev.answers()[2])


def best_kp_changed(dev, s):
    dev.matched[s]["best_kp"][0] += 1
    return dev.answers()


def proj_nan(dev, s):
    at = np.argwhere(~np.isnan(dev.matched[s]["proj_yx"]))[0]
    dev.matched[s]["proj_yx"][tuple(at)] = np.nan
    return dev.answers()


@pytest.mark.parametrize("proj_tol", (0.0, kd.PX_TOL))
@pytest.mark.parametrize("mutant", (pairs_int32, best_kp_changed, proj_nan), ids=lambda f: f.__name__)
def test_check_match_catches_one_changed_answer(rows_run, mutant, proj_tol):
    r, dev = rows_run.stand_in(proj_tol=proj_tol)
    s = next(s for s, w in enumerate(rows_run.matched) if len(w["lm_ids"]) and not np.all(np.isnan(w["proj_yx"])))
    got = mutant(dev, s)
    with pytest.raises(AssertionError):
        rows_run.check_match(got, rows_run.matched)


def _windows(h):
    """the model's windows of the present state and the device's Window records of the same, as KeyframeMap.gather returns them"""
    ref = {s: w for s in range(len(h.m)) for w in [npk.gather(copy.deepcopy(h.m[s]))] if w is not None}
    wins = [SimpleNamespace(stream=s, cache=SimpleNamespace(**{key: w[key].copy() for key in ("theta", "theta_const", "pixels", "poses_ids", "points_ids")}),
                            **{key: w[key].copy() for key in ("poses_remap", "points_remap", "obs_kf", "obs_kp", "obs_in_covmap")}) for s, w in sorted(ref.items())]
    return ref, wins, np.array([0 if s in ref else 1 for s in range(len(h.m))], dtype=np.int32)


@pytest.mark.parametrize("px_tol", (0.0, kd.PX_TOL))
def test_check_windows_catches_a_moved_angle_and_another_dtype(rows_run, px_tol):
    h = rows_run
    h.stand_in(px_tol)
    ref, wins, status = _windows(h)
    assert wins
    h.check_windows(wins, status, ref)
    wins[0].cache.theta[0] += 1e-9                               # an angle of the window's first pose
    with pytest.raises(AssertionError):
        h.check_windows(wins, status, ref)
    ref, wins, status = _windows(h)
    wins[-1].obs_kf = wins[-1].obs_kf.astype(np.int32)           # equal values, another dtype
    with pytest.raises(AssertionError):
        h.check_windows(wins, status, ref)
    ref, wins, status = _windows(h)
    status[0] = 3
    with pytest.raises(AssertionError):
        h.check_windows(wins, status, ref)
