"""GPU: the key-frame map at the ring's limits -- R = 2, the smallest ring, and R = 64, where a wrapped ring uses bit 63 of every 64-bit observer mask,
covisibility mask and removal mask -- with S = 2, cap = 65 and mcap = 130 (no multiple of 64: the last word of every stored set is partial, and the
table wraps several times).  The scenes are tests/kfmap_history_scripts.py's (seeds 21, 22) made 70 key-frames long for R = 64 and 6 for R = 2; on
alternate key-frames one of the two streams is not selected, so the streams' rings stand at different slots.  Every key-frame: add_keyframe +
add_descriptors -> local_map_match with the history -> merge of the match's pairs where they lie in HBM; behind some a gather + update, behind some a
filter.  After EVERY call the device equals the numpy models (np_kfmap, np_kfmap_filter, np_kfmap_local_map_history, np_kfmap_merge): statuses, pairs,
distances, staged lists, merge counts, gathered windows, removed key-frames, every key-frame of the ring (download_keyframe), the points
(download_points) and every stored local map (local_map_ids) array_equal; a key-frame's angles to 1e-12 (computed on the device, then handed to the
model) and proj_yx to 1e-9 px, as in tests/test_gpu_kfmap.py and tests/test_gpu_kfmap_local_map_history.py.

test_the_models_alone_reach_the_edges runs the same sequence on the models alone, without a GPU, and shows what it reaches."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_history_scripts as hs  # noqa: E402
import kfmap_lmm_scripts as ls  # noqa: E402
import np_kfmap_filter as npf  # noqa: E402

S, CAP, MCAP, DCAP, MINC = 2, 65, 130, 65, 4
N_KF = {2: 6, 64: 70}
PX_TOL, ANGLE_TOL = 1e-9, 1e-12


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


class Pair(Run):
    """the device map with its keypoint set beside the models"""

    def __init__(self, slam, R):
        import torch
        self.torch, self.slam = torch, slam
        super().__init__(R)
        self.ks = slam.KeypointSet(S, CAP)
        self.km = slam.KeyframeMap(S, CAP, R=R, mcap=MCAP)
        self.km.enable_descriptors()
        self.km.enable_local_map_history()
        self.Tcw = np.tile(np.eye(4), (S, 1, 1))

    def close(self):
        self.km.close(); self.ks.close()

    def add(self, mask=None):
        took = super().add(mask)
        desc = np.full((S, DCAP, 4), 0x5555555555555555, dtype=np.uint64)
        info = np.tile(np.array([10 ** 6, 3], dtype=np.int64), (S, 1))
        for s, (f, d) in took.items():
            self.ks.upload(s, f["yx"], f["is_3d"], f["xyz"], f["ids"])
            self.Tcw[s] = f["Tcw"]
            info[s] = (d[0], len(d[1])); desc[s, :len(d[1])] = d[1]
        sp = self.slam.stream_params(S, Tcw=self.Tcw, cam=ls.CAM10[:4], dist=np.zeros((S, 4)))
        desc_dev = self.torch.from_numpy(desc.view(np.int64)).cuda(); info_dev = self.torch.from_numpy(info).cuda()
        with self.ks.selected(mask):
            self.ks.keyframe()
            self.km.add_keyframe(self.ks, sp)
            self.km.add_descriptors(desc_dev.data_ptr(), info_dev.data_ptr(), DCAP)
        self.km.ctx.synchronize()
        for s in took:                                           # the device's angles, checked to their bar, become the model's
            k = self.nkf[s] - 1
            th, ref = self.km.download_keyframe(s, k)["theta"], self.m[s].theta[k % self.R]
            assert np.array_equal(th[3:], ref[3:]) and np.all(np.abs(th[:3] - ref[:3]) <= ANGLE_TOL), (s, k)
            self.m[s].theta[k % self.R] = th
        return took

    def match(self, max_local=None, **kw):
        want = super().match(max_local=max_local, **kw)
        status, pairs, dist = self.km.local_map_match(ls.CAM10, ls.CELL, ls.PARAMS.max_projection_distance, ls.PARAMS.max_descriptor_distance, max_local=max_local)
        assert list(status) == [w["status"] for w in want]
        for s in range(S):
            w = want[s]
            assert w["margin"] >= 1e-9
            assert pairs[s].dtype == np.int64 and np.array_equal(pairs[s], w["pairs"]) and np.array_equal(dist[s], w["dist"]), s
            if not self.sel[s]:
                continue
            d = self.km.debug_local_map(s)
            assert np.array_equal(d["lm_ids"], w["lm_ids"]) and np.array_equal(d["kp_ids"], w["kp_ids"]), s
            assert np.array_equal(d["best_kp"], w["best_kp"]) and np.array_equal(d["best_dist"], w["best_dist"]), s
            assert np.array_equal(np.isnan(d["proj_yx"]), np.isnan(w["proj_yx"])), s
            ok = ~np.isnan(w["proj_yx"])
            assert np.all(np.abs(d["proj_yx"][ok] - w["proj_yx"][ok]) <= PX_TOL), s
        return want

    def merge(self, pairs):
        want = super().merge(pairs).copy()
        got = self.km.merge(None, None)
        assert np.array_equal(got, want), (got, want)
        return want

    def ba(self):
        wins, status = self.km.gather(np.full(S, MINC, dtype=np.int32))
        sol = super().ba()
        assert list(status) == [3 if not self.sel[s] else (0 if s in sol else 1) for s in range(S)]
        assert [w.stream for w in wins] == sorted(sol)
        for w in wins:
            ref, c = sol[w.stream][0], w.cache
            P = len(ref["poses_remap"])
            for a, b in ((c.theta_const, ref["theta_const"]), (c.poses_ids, ref["poses_ids"]), (c.points_ids, ref["points_ids"]), (w.poses_remap, ref["poses_remap"]),
                         (w.points_remap, ref["points_remap"]), (w.obs_kf, ref["obs_kf"]), (w.obs_kp, ref["obs_kp"]), (w.obs_in_covmap, ref["obs_in_covmap"]),
                         (c.pixels, ref["pixels"]), (c.theta, ref["theta"])):
                assert a.dtype == b.dtype and np.array_equal(a, b), w.stream      # (the poses' angles are the device's own bits: add() gave them to the model)
            assert P >= 1 and c.poses_ids.min() >= 1 and c.points_ids.min() >= 1
        self.km.update(wins, [sol[w.stream][1] for w in wins], [sol[w.stream][2] for w in wins])
        return sol

    def filter(self):
        ratio, minc = self.filter_args()
        got = self.km.filter(ratio, np.array(minc, dtype=np.int32), first_kfid=0)
        want, logs = super().filter()
        assert got == want, (got, want)
        return want, logs

    def check(self):
        """every key-frame the ring can hold, the points and the stored sets of every stream against the models"""
        for s, m in enumerate(self.m):
            for k in range(max(self.nkf[s] - self.R, 0), self.nkf[s] + 1):
                d, w = self.km.download_keyframe(s, k), m.keyframe(k)
                assert (d is None) == (w is None), (s, k)
                if w is not None:
                    assert all(np.array_equal(d[key], w[key]) for key in ("theta", "ids", "upx", "live")), (s, k)
                try:
                    got = self.km.local_map_ids(s, k)
                except self.slam.SlamHipError as e:
                    got = str(e)
                want = self.H[s].ids(m, k)
                if want is None:
                    assert isinstance(got, str) and ("not in the ring" in got or "no local map was stored" in got), (s, k, got)
                else:
                    assert not isinstance(got, str) and got.dtype == np.int64 and np.array_equal(got, want), (s, k)
            d, w = self.km.download_points(s), m.points()
            assert all(np.array_equal(d[key], w[key]) for key in ("ids", "xyz", "is_3d", "observed", "ba", "gone")) and d["observers"] == w["observers"], s


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
