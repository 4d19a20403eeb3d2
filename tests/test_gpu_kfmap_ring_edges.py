"""GPU: the key-frame map at the ring's limits -- R = 2, the smallest ring, and R = 64, where a wrapped ring uses bit 63 of every 64-bit observer mask,
covisibility mask and removal mask -- with S = 2, cap = 65 and mcap = 130 (no multiple of 64: the last word of every stored set is partial, and the
table wraps several times).  The scenes are tests/kfmap_history_scripts.py's (seeds 21, 22) made 70 key-frames long for R = 64 and 6 for R = 2; on
alternate key-frames one of the two streams is not selected, so the streams' rings stand at different slots.  Every key-frame: add_keyframe +
add_descriptors -> local_map_match with the history -> merge of the match's pairs where they lie in HBM; behind some a gather + update, behind some a
filter.  After EVERY call the device equals the numpy models (np_kfmap, np_kfmap_filter, np_kfmap_local_map_history, np_kfmap_merge): statuses, pairs,
distances, staged lists, merge counts, gathered windows, removed key-frames, every key-frame of the ring (download_keyframe), the points
(download_points) and every stored local map (local_map_ids) array_equal; a key-frame's angles to 1e-12 (computed on the device, then handed to the
model, as in tests/test_gpu_kfmap.py) and proj_yx to 1e-9 px.  The device side of every step and every comparison are tests/kfmap_device.py's.

test_the_models_alone_reach_the_edges runs the same sequence on the models alone, without a GPU, and shows what it reaches."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_device as kd  # noqa: E402
import kfmap_history_scripts as hs  # noqa: E402
import np_kfmap_filter as npf  # noqa: E402

S, CAP, MCAP, DCAP, MINC = 2, 65, 130, 65, 4
N_KF = {2: 6, 64: 70}


def sizes(n_kf):
    """list lengths around 30, with 0, 1, 64 and 65 (= cap) among them where the sequence is long enough"""
    out = [[24 + (7 * k + 5 * s) % 13 for k in range(n_kf)] for s in range(S)]
    for k, v in ((9, 65), (17, 0), (18, 1), (33, 64), (50, 65)):
        if k < n_kf:
            out[k % S][k] = v
    return tuple(tuple(o) for o in out)


def mask_at(k, nkf, n_kf):
    """on alternate key-frames one stream is not selected, in turn; a stream that has taken its last scripted key-frame is no longer selected"""
    left = tuple(int(n < n_kf) for n in nkf)
    turn = (1,) * S if k % 2 == 0 else ((1, 0) if k % 4 == 1 else (0, 1))
    both = tuple(a & b for a, b in zip(left, turn))
    return both if any(both) else left


class Run(hs.HistoryRun):
    """the models of the two streams"""

    def __init__(self, R):
        super().__init__(R=R, mcap=MCAP, cap=CAP, sizes=sizes(N_KF[R]), window=6)
        assert self.n == S and all(m.min_cov_score == MINC for m in self.m)
        self.R = R

    def filter_args(self):
        """per stream a min_cov_score that removes the covisible key-frame with the fewest 3-D points (np_kfmap_filter's `few` rule), where there is one"""
        minc = []
        for s in range(S):
            log = npf.filter_map(copy.deepcopy(self.m[s]), 0.999999, 0, first_kfid=0) if self.sel[s] else []
            minc.append(2 * (min([t for _, ex, t, _ in log if ex != "break"], default=-1) + 1))
        return 0.999999, minc

    def filter(self):
        ratio, minc = self.filter_args()
        logs = [npf.filter_map(self.m[s], ratio, minc[s], first_kfid=0) if self.sel[s] else [] for s in range(S)]
        return [sorted(k for k, ex, _, _ in log if ex in ("few", "ratio")) for log in logs], logs


def run_edges(run, on_step=None):
    """every key-frame add -> match (max_local = mcap: status 2 cannot occur) -> merge; behind every third a gather + update, behind every fifth a filter"""
    k = -1
    while min(run.nkf) < N_KF[run.R]:
        k += 1
        took = run.add(mask_at(k, run.nkf, N_KF[run.R]))
        on_step and on_step("add", k, took)
        res = run.match(max_local=MCAP)
        on_step and on_step("match", k, res)
        run.merge(hs.pairs_of(res))
        on_step and on_step("merge", k, None)
        if k % 3 == 2:
            on_step and on_step("ba", k, run.ba())
        if k % 5 == 4:
            on_step and on_step("filter", k, run.filter())


@pytest.mark.parametrize("R", sorted(N_KF))
def test_the_models_alone_reach_the_edges(R):
    """no GPU: the sequence on the models -- the ring wraps (R = 64: slot 63 holds the newest key-frame, and in turn an observer and a covisible one), the
    table wraps, pairs, windows and removals occur on both streams"""
    run = Run(R)
    seen = dict(pairs=[0] * S, wins=[0] * S, removed=[0] * S, top_obs=0, top_cov=0, sizes=set(), apart=0)

    def on_step(kind, k, data):
        seen["apart"] += kind == "add" and run.nkf[0] % R != run.nkf[1] % R           # the two rings stand at different slots
        for s in range(S):
            if kind == "add" and s in data:
                seen["sizes"].add(len(data[s][0]["ids"]))
                seen["top_obs"] += any(m >> (R - 1) & 1 for m in run.m[s].mask) and run.m[s].cur % R != R - 1
            if kind == "match":
                seen["pairs"][s] += len(data[s]["pairs"])
                seen["top_cov"] += run.sel[s] and (R - 1) in hs.nh.nl.covisible_slots(run.m[s])
            if kind == "ba":
                seen["wins"][s] += s in data
            if kind == "filter":
                seen["removed"][s] += len(data[0][s])
    run_edges(run, on_step)
    assert run.nkf == [N_KF[R]] * S and seen["apart"] >= N_KF[R] // 2
    assert all(max(int(t) for t in m.ptag) >= (3 * MCAP if R == 64 else 0) for m in run.m)
    if R == 64:
        assert min(run.nkf) > R and {0, 1, 64, 65} <= seen["sizes"]
        assert min(seen["pairs"]) >= 20 and min(seen["wins"]) >= 5 and min(seen["removed"]) >= 2, seen
        assert seen["top_obs"] >= 1 and seen["top_cov"] >= 1, seen
        assert all(h.count["purged"] >= 10 and h.count["chained"] >= 3 for h in run.H)
    else:
        assert sum(seen["pairs"]) >= 1 and sum(seen["wins"]) >= 1, seen


class Pair(kd.DeviceSide, Run):
    """the device map with its keypoint set beside the models"""
    dcap = DCAP
    device_pairs = True                                          # merge(): the pairs the last match left in HBM
    proj_tol = kd.PX_TOL                                         # staged proj_yx: the device's sines and cosines of a late key-frame's angles differ in the last place

    def __init__(self, slam, R):
        super().__init__(slam, R, lm_history=True)

    def filter(self):
        ratio, minc = self.filter_args()
        got = self.km.filter(ratio, np.array(minc, dtype=np.int32), first_kfid=0)
        want, logs = super().filter()
        assert got == want, (got, want)
        return want, logs


@pytest.mark.gpu
@pytest.mark.parametrize("R", sorted(N_KF))
def test_device_equals_models_after_every_call_at_the_rings_limits(slam, R):
    p = Pair(slam, R)
    try:
        steps = set()

        def on_step(kind, k, data):
            steps.add(kind)
            p.check()
        run_edges(p, on_step)
        assert steps == {"add", "match", "merge", "ba", "filter"}
    finally:
        p.close()
