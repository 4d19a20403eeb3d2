"""Scripted sequences for the local-map history of the key-frame map (test helper): the scenes of tests/kfmap_lmm_scripts.py, made longer and with a
wider copy window, so that a copy is born after every key-frame that observes its original has stopped being covisible with the newest one -- the
"lost long ago, seen again" case that only the chain of stored local maps (tests/np_kfmap_local_map_history.py) brings back to the match.

The main scene: S = 3 (seeds 21-23), cap 64, R = 6, mcap = 128, 12 key-frames of 40 + (7 k + 3 s) % 9 keypoints, copies of points lost up to 6 key-frames
ago; every key-frame add -> match -> merge of the match's pairs (no keypoint set: later lists still carry the prev ids), a local-BA update behind
key-frames 3 and 4.  tests/test_kfmap_local_map_history_host.py shows what it reaches."""
import copy

import numpy as np

import kfmap_lmm_scripts as ls
import kfmap_merge_scripts as ms
import np_kfmap_filter as npf
import np_kfmap_local_map_history as nh

S, CAP, R, MCAP, N_KF, WINDOW = 3, 64, 6, 128, 12, 6
SIZES = tuple(tuple(40 + (7 * k + 3 * s) % 9 for k in range(N_KF)) for s in range(S))
BA_AT = ls.BA_AT
TWO_CALLS_AT = 8                         # the key-frame behind which the match runs again (two_calls)


class HistoryRun(ms.MergeRun):
    """MergeRun (mode "stale") on the main scene with a History per stream; match() is the model WITH history (history=False: np_kfmap_local_map's)"""

    def __init__(self, R=R, mcap=MCAP, cap=CAP, sizes=SIZES, window=WINDOW, history=True):
        frames, descs = ls.scenes(sizes=sizes, window=window)
        ls.ModelRun.__init__(self, frames, descs, R=R, mcap=mcap, cap=cap)
        self.mode = "stale"
        self.lists = [None] * self.n
        self.ren = [dict() for _ in range(self.n)]
        self.log = [dict() for _ in range(self.n)]
        self.counts = np.zeros((self.n, 4), dtype=np.int32)
        self.history = history
        self.H = [nh.History(R) for _ in range(self.n)]

    def match(self, max_local=None, mutant=None, H=None):
        """H: the histories to use and change (default: the run's own)"""
        if not self.history:
            return ls.ModelRun.match(self, max_local=max_local)
        H = self.H if H is None else H
        idle = dict(nh._none(), C=[], size=0, chain=[], branch=None)
        return [nh.local_map_match(self.m[s], self.D[s], H[s], ls.CAM10, ls.CELL, ls.PARAMS, max_local=max_local, mutant=mutant) if self.sel[s] else idle
                for s in range(self.n)]

    def remove_keyframe(self, s, kfid):
        npf.remove_keyframe(self.m[s], kfid)

    def reset(self, s):
        """slam_kfmap_reset on the model: an empty ring and table, no descriptors, no history (the scripted sequence of the stream goes on)"""
        import np_kfmap as npk
        import np_kfmap_local_map as nl
        old = self.m[s]
        self.m[s] = npk.Map(old.cap, old.R, old.mcap, ls.CAM10[:4], None, old.min_cov_score)
        self.D[s] = nl.new_descriptors(self.m[s])
        self.H[s].reset()


def pairs_of(res):
    return [r["pairs"] if r["status"] == 0 else np.zeros((0, 2), dtype=np.int64) for r in res]


def run_sequence(run, n_kf=N_KF, merges=True, on_step=None, max_local=None):
    """every key-frame add -> match -> (merge of the match's pairs) -> behind key-frames 3 and 4 a gather + update; on_step(kind, k, data) after each"""
    for k in range(n_kf):
        took = run.add()
        on_step and on_step("add", k, took)
        res = run.match(max_local=max_local)
        on_step and on_step("match", k, res)
        if merges:
            run.merge(pairs_of(res))
            on_step and on_step("merge", k, pairs_of(res))
        if k in BA_AT:
            sol = run.ba()
            on_step and on_step("ba", k, sol)


def covisible_ids(run, s):
    import np_kfmap_local_map as nl
    m = run.m[s]
    return sorted(int(m.tag[b]) for b in nl.covisible_slots(m))


def plan_second_call(run, s, want):
    """which covisible key-frames of stream s to remove so that a second match for the same key-frame takes the `want` branch ("union": C shrinks to at
    most half of the stored set; "replace": it stays above half) -> the list of key-frame ids, or None where the stream cannot show it.  Tried on
    copies: the run is not changed."""
    cov = covisible_ids(run, s)
    for n in range(1, len(cov) + 1):
        for drop in ([cov[-n:], cov[:n]] if n < len(cov) else [cov]):
            m, H = copy.deepcopy(run.m[s]), copy.deepcopy(run.H[s])
            for k in drop:
                npf.remove_keyframe(m, k)
            r = nh.local_map_match(m, run.D[s], H, ls.CAM10, ls.CELL, ls.PARAMS)
            if r["branch"] == want:
                return list(drop)
    return None
