"""GPU: the work records of a match (KpWorkRec: k_kpset_worklist hands k_kpset_match everything its prologue used to look up -- csrc/kpset.hpp,
csrc/work_order.hpp) change how a wave of k_kpset_match learns its keypoint, never what the lists hold.  SLAMHIP_NO_MATCH_REC is read once per
process, so every setting runs in a child process of its own (the six start together) and leaves its lists in an .npz file:
    knob unset / 1   x   {default, SLAMHIP_LK_GRID=8 (the multi-round loop), SLAMHIP_WORK_BAND=0 (slot order)}
Every child runs, for S = 1, 3 and 9 streams of 96 x 128 frames (pyramid_levels 3, window 9, cap 48):
  stage u<prior>  uploaded lists (lengths 0, 1 and cap among the streams; 2-D and 3-D keypoints, some 3-D ones with a prior far outside the
                  image) through a temporal match, a stereo match and the triangulation, for prior 0, 1 and 2;
  stage c         two key-frame periods of the cycle from empty lists (prior 2); the second key-frame acts on a strict subset of the streams
                  (slam_kpset_select), then a stereo match with no stream selected;
  stage tol       (S = 9) stage u2 on tolerance-mode pyramids (the contracted-arithmetic instantiation);
  stage host      (S = 3) the temporal match of stage u2 again through the host-list seam slam_flow_match_batch_kept, which never sees a record.
Asserted: every field of every list after every step byte-equal between the knob's two settings (and across the three environments); the
host-list seam's survivors and positions byte-equal to the set's; and, first, that the case does real work -- every path taken by at least
one keypoint."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("yx", "is_3d", "xyz", "ids", "stereo_yx", "has_stereo")
ENVS = {"default": {}, "grid8": {"SLAMHIP_LK_GRID": "8"}, "slot_order": {"SLAMHIP_WORK_BAND": "0"}}
KNOBS = {"rec": None, "norec": "1"}
SIZES = (1, 3, 9)
CAP, H, W = 48, 96, 128

CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
import slam_jl_amd as slam
from slam_jl_amd import synthetic as syn
H, W, CAP, LEVELS, KF, NT = 96, 128, 48, 3, 5, 11
params = slam.Params(stereo=True, max_nb_keypoints=24)
assert params.pyramid_levels == 3 and params.window_size == 9
cam = slam.Camera(*syn.KITTI_CAM, height=H, width=W)
ex = slam.Extractor.from_params(params, cam)
assert ex.max_points + ex.grid_resolution[0] * ex.grid_resolution[1] + 8 <= CAP
fx, fy, cx, cy = syn.KITTI_CAM
disparity, step = 5.0, (1.7, -2.9)
out = {}
keep_alive = []
u8 = lambda im: np.ascontiguousarray(np.round(im * 255).astype(np.uint8).T)
LENGTHS = {1: (CAP,), 3: (0, 1, CAP), 9: (CAP, 0, 1, 17, CAP, 5, 0, 33, CAP)}

def run(S):
    left, right, flows = syn.stereo_stream((H, W), NT + S, seed=40 + S, step=step, disparity=disparity)
    flows = np.asarray(flows)
    def batch(frames, t, **kw):
        d = torch.from_numpy(np.stack([u8(frames[t + s]) for s in range(S)])).cuda(); torch.cuda.synchronize(); keep_alive.append(d)
        b = slam.PyramidBatch((H, W), levels=LEVELS, S=S)
        b.update_([d.data_ptr() + s * H * W for s in range(S)], u8=True, **kw)
        return b
    rng = np.random.default_rng(100 + S)
    ks = slam.KeypointSet(S, CAP)
    def dump(tag):
        for s in range(S):
            d = ks.download(s)
            for f in %(fields)r:
                out["S%%d_%%s_s%%d_%%s" %% (S, tag, s, f)] = d[f]
        out["S%%d_%%s_counts" %% (S, tag)] = ks.counts()
    T21 = np.eye(4); T21[0, 3] = -disparity * 30.0 / fx
    flow1 = flows[1] - flows[0]                                  # every stream moves by the same step between two frames
    def lists():
        """per stream: positions inside the image (some close to its border), 60 %% 3-D; a quarter of the 3-D ones get a map point / sit
        where the prior of every mode-1 / mode-2 match falls far outside the image"""
        L = []
        for s, n in enumerate(LENGTHS[S]):
            yx = np.stack([rng.uniform(2, H - 1, n), rng.uniform(8, W - 1, n)], axis=1)
            is3 = rng.random(n) < 0.6
            far = is3 & (rng.random(n) < 0.25)
            if n == CAP:
                is3[:4] = [True, True, False, False]; far[:4] = [True, False, False, False]     # the full lists hold every kind
                yx[2] = (H - 0.6, 40.0)                            # a 2-D keypoint the flow (+1.7 rows) carries out of the image: lost
            yx[far, 1] = rng.uniform(1.2, 2.5, int(far.sum()))     # x + shift_x < 1 under both shifts (temporal -2.9, stereo -5.0): outside for prior 2
            tgt = yx + flow1
            tgt[far] = yx[far] + np.array([0.0, -60.0])           # and its map point projects 60 px left of the image: outside for prior 1
            z = rng.uniform(5, 30, n)
            xyz = np.stack([(tgt[:, 1] - cx) / fx * z, (tgt[:, 0] - cy) / fy * z, z], axis=1)   # camera = world (Tcw = I)
            L.append((yx, is3, xyz, far))
        return L
    def stage_u(tag, prior, b0, b1, r1):
        L = lists()
        for s, (yx, is3, xyz, far) in enumerate(L):
            ks.upload(s, yx, is3, xyz=xyz)
            out["S%%d_%%s_pre_s%%d_yx" %% (S, tag, s)] = yx; out["S%%d_%%s_pre_s%%d_is3" %% (S, tag, s)] = is3; out["S%%d_%%s_pre_s%%d_far" %% (S, tag, s)] = far
        sp_t = slam.stream_params(S, Tcw=np.eye(4), cam=syn.KITTI_CAM, shift_yx=np.tile(flow1, (S, 1)))
        sp_s = slam.stream_params(S, Tcw=np.eye(4), cam=syn.KITTI_CAM, shift_yx=np.tile([0.0, -disparity], (S, 1)))
        ks.flow_match(b0, b1, params, sp_t, prior=prior)
        dump(tag + "_match")
        ks.stereo_match(b1, r1, params, sp_s, prior=prior)
        dump(tag + "_stereo")
        ks.triangulate(syn.KITTI_CAM, syn.KITTI_CAM, T21, np.eye(4), max_error=3.0)
        dump(tag + "_tri")
        return L
    b0, b1, r1 = batch(left, 0), batch(left, 1), batch(right, 1, target_only=True)
    for prior in (0, 1, 2):
        L = stage_u("u%%d" %% prior, prior, b0, b1, r1)
    if S == 3:
        # stage host: the temporal match of stage u2 (the lists just used) through the host-list seam
        P = np.concatenate([l[0] for l in L]); T = np.concatenate([l[1] for l in L]); I = np.concatenate([np.full(len(l[0]), s, np.int32) for s, l in enumerate(L)])
        proj = P + flow1
        inside = (proj[:, 0] >= 1) & (proj[:, 0] <= H) & (proj[:, 1] >= 1) & (proj[:, 1] <= W)
        skip = T & ~inside                                       # map_manager.jl:501-506: left as they are
        hk, h3, hs, hsrc = slam.optical_flow_matching_batch_kept(b0, b1, I[~skip], P[~skip], T[~skip], proj[~skip], params)
        pos = np.full((len(P), 2), np.nan); alive = np.zeros(len(P), bool)
        idx_ns = np.flatnonzero(~skip)
        pos[idx_ns[hsrc]] = hk; alive[idx_ns[hsrc]] = True
        pos[skip] = P[skip]; alive[skip] = True
        for s in range(S):
            m = (I == s) & alive
            out["S3_host_s%%d_yx" %% s] = pos[m]; out["S3_host_s%%d_is3" %% s] = T[m]
        out["S3_host_skipped"] = np.array([int(skip.sum())]); out["S3_host_lost"] = np.array([int((~alive).sum())])
    if S == 9:
        t0, t1, tr = batch(left, 0, fast=True), batch(left, 1, fast=True), batch(right, 1, fast=True)
        stage_u("tol", 2, t0, t1, tr)
    # stage c: two key-frame periods from empty lists; the second key-frame under a selection
    for s in range(S):
        ks.upload(s, np.zeros((0, 2)), np.zeros(0, bool))
    subset = np.arange(S) %% 3 == 1                                # a strict subset (no stream at S = 1)
    sp_stereo = slam.stream_params(S, cam=syn.KITTI_CAM, shift_yx=np.tile([0.0, -disparity], (S, 1)))
    prev = None
    for t in range(1, NT):
        cur = batch(left, t)
        if prev is not None and ks.counts().sum() > 0:
            sh = np.array([flows[t + s] - flows[t - 1 + s] for s in range(S)]) + rng.normal(0, 0.5, (S, 2))
            ks.flow_match(prev, cur, params, slam.stream_params(S, cam=syn.KITTI_CAM, shift_yx=sh), prior=2, n_bound=int(ks.counts().sum()))
        if (t - 1) %% KF == 0:
            fl = torch.from_numpy((rng.random(S * CAP) < 0.15).astype(np.uint8)).cuda(); torch.cuda.synchronize(); keep_alive.append(fl)
            ks.remove(fl.data_ptr())
            rt = batch(right, t, target_only=True)
            with ks.selected(None if t == 1 else subset):
                ks.detect(ex, cur)
                ks.stereo_match(cur, rt, params, sp_stereo, prior=2)
                ks.triangulate(syn.KITTI_CAM, syn.KITTI_CAM, T21, np.eye(4), max_error=3.0)
            if t > 1:
                dump("c_sub%%d" %% t)
                with ks.selected(np.zeros(S, bool)):
                    ks.stereo_match(cur, rt, params, sp_stereo, prior=2)      # no stream selected: nothing may change
        dump("c%%d" %% t)
        prev = cur
    ks.close()

for S in %(sizes)r:
    run(S)
np.savez(%(path)r, **out)
print("OK")
'''


def _spawn(code, env_extra, knob):
    env = dict(os.environ)
    for k in ("SLAMHIP_NO_MATCH_REC", "SLAMHIP_LK_GRID", "SLAMHIP_WORK_BAND", "SLAMHIP_NO_TOL_LK"):
        env.pop(k, None)
    env.update(env_extra)
    if knob is not None:
        env["SLAMHIP_NO_MATCH_REC"] = knob
    return subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("match_records")
    keys = [(e, k) for e in ENVS for k in KNOBS]
    paths = {key: str(d / ("%s_%s.npz" % key)) for key in keys}
    procs = {key: _spawn(CHILD % dict(root=ROOT, fields=FIELDS, sizes=SIZES, path=paths[key]), ENVS[key[0]], KNOBS[key[1]]) for key in keys}
    for p in procs.values():
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0 and so.strip().endswith("OK"), so[-800:] + se[-2000:]
    return {key: dict(np.load(paths[key])) for key in keys}


def _lengths(S):
    return {1: (CAP,), 3: (0, 1, CAP), 9: (CAP, 0, 1, 17, CAP, 5, 0, 33, CAP)}[S]


def test_the_case_does_real_work(runs):
    """counted in the record-less run (the behaviour before there were records): every path is taken by at least one keypoint"""
    a = runs[("default", "norec")]
    for S in SIZES:
        assert sorted(set(_lengths(S))) == sorted(set(len(a["S%d_u0_pre_s%d_yx" % (S, s)]) for s in range(S)))      # lists of 0, 1 and cap keypoints (S = 1: cap)
        for tag in ("u0", "u1", "u2") + (("tol",) if S == 9 else ()):
            n = dict(two_d=0, three_d=0, far=0, lost=0, tracked=0, skipped=0, stereo_in=0, stereo_ok=0, stereo_fail=0, stereo_far=0, tri=0)
            for s in range(S):
                pre_yx, is3, far = (a["S%d_%s_pre_s%d_%s" % (S, tag, s, f)] for f in ("yx", "is3", "far"))
                ids = a["S%d_%s_match_s%d_ids" % (S, tag, s)]; yx = a["S%d_%s_match_s%d_yx" % (S, tag, s)]
                n["two_d"] += int((~is3).sum()); n["three_d"] += int((is3 & ~far).sum()); n["far"] += int(far.sum())
                n["lost"] += len(pre_yx) - len(ids)
                moved = (yx != pre_yx[ids]).any(axis=1)
                n["tracked"] += int(moved.sum())
                if tag != "u0":                                  # prior 0 is the pixel itself: never outside
                    assert far[ids].sum() == far.sum() and not moved[far[ids]].any(), (S, tag, s)     # skipped: kept as they are
                    n["skipped"] += int(far[ids].sum())
                st_ids = a["S%d_%s_stereo_s%d_ids" % (S, tag, s)]; hs = a["S%d_%s_stereo_s%d_has_stereo" % (S, tag, s)]
                n["stereo_in"] += len(ids); n["stereo_ok"] += int(hs.sum()); n["stereo_fail"] += int((~hs).sum())
                n["stereo_far"] += len(ids) - len(st_ids) if tag != "u0" else 0        # a 3-D keypoint projected outside the right image (st = 0)
                n["tri"] += int(a["S%d_%s_tri_s%d_is_3d" % (S, tag, s)].sum() - a["S%d_%s_stereo_s%d_is_3d" % (S, tag, s)].sum())
            need = ["two_d", "three_d", "lost", "tracked", "stereo_in", "stereo_ok", "stereo_fail"] + ([] if tag == "u0" else ["far", "skipped", "stereo_far"])
            print(S, tag, n)
            assert all(n[k] > 0 for k in need), (S, tag, n)
        # the cycle: lists of several generations, a selection that acts on a strict subset
        c = [a["S%d_c%d_counts" % (S, t)] for t in range(1, 11)]
        assert c[0].min() > 5 and c[9].sum() > 0, (S, c)
        subset = np.arange(S) % 3 == 1
        before, after = a["S%d_c5_counts" % S], a["S%d_c_sub6_counts" % S]
        if subset.any():
            assert (after[subset] > 0).all(), (S, before, after)
            for s in np.flatnonzero(subset):
                assert a["S%d_c_sub6_s%d_has_stereo" % (S, s)].any(), (S, s)                       # the selected streams' stereo match did match
        for s in np.flatnonzero(~subset):
            assert after[s] <= before[s], (S, s)                                               # no detection in an unselected stream
        for s in range(S):                                                                     # no stream selected: the stereo match changed nothing
            for f in FIELDS:
                assert a["S%d_c_sub6_s%d_%s" % (S, s, f)].tobytes() == a["S%d_c6_s%d_%s" % (S, s, f)].tobytes(), (S, s, f)
    assert a["S3_host_skipped"][0] > 0 and a["S3_host_lost"][0] > 0


@pytest.mark.parametrize("env", list(ENVS))
def test_same_lists_with_and_without_records(runs, env):
    a, b = runs[(env, "norec")], runs[(env, "rec")]
    assert a.keys() == b.keys() and len(a) > 1000
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (env, k)


@pytest.mark.parametrize("env", ["grid8", "slot_order"])
def test_same_lists_in_every_environment(runs, env):
    """the multi-round loop and the slot-order walk read the records at other places and times: the same lists as the default launch"""
    a, b = runs[("default", "rec")], runs[(env, "rec")]
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (env, k)


@pytest.mark.parametrize("knob", list(KNOBS))
def test_temporal_match_equals_the_host_list_seam(runs, knob):
    """slam_flow_match_batch_kept takes host lists and never sees a record: survivors, their order and positions byte-equal to the set's"""
    a = runs[("default", knob)]
    for s in range(3):
        assert a["S3_u2_match_s%d_yx" % s].tobytes() == a["S3_host_s%d_yx" % s].tobytes(), (knob, s)
        assert np.array_equal(a["S3_u2_match_s%d_is_3d" % s], a["S3_host_s%d_is3" % s]), (knob, s)
