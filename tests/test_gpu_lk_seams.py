"""GPU: the six entry points of the tracking kernels (fb_tracking_, optical_flow_matching, _batch, _batch_kept, KeypointSet.flow_match,
.stereo_match) share one per-point body and one set of preconditions (csrc/lk.hip: fb_point, lk_launch, match_check): the same lists
through every seam give the same tracks bit for bit, on the 6- and 9-slot instantiations too, and every seam refuses the same
pyramids with the same error, in the same order, before anything is launched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, H, W = 3, 120, 160


@pytest.fixture(scope="module")
def scene(slam, orc, texture):
    """three streams with ragged lists (detections + three border points, about half of them 3-D), as test_gpu_kpset.py builds them; the
    prior shift is the true flow for streams 0 and 1 and the true flow + (0, 40) for stream 2: its 3-D keypoints fail the prior attempt"""
    import torch
    streams = [texture(H, W, seed=30 + s, step=(1.0 + 0.2 * s, -1.4), disparity=6.3) for s in range(S)]
    a = slam.PyramidBatch((H, W), levels=3, S=S); b = slam.PyramidBatch((H, W), levels=3, S=S)
    d0 = [torch.from_numpy(np.ascontiguousarray(st[0][0].T)).cuda() for st in streams]
    d1 = [torch.from_numpy(np.ascontiguousarray(st[0][1].T)).cuda() for st in streams]
    torch.cuda.synchronize()
    a.update_([d.data_ptr() for d in d0]); b.update_([d.data_ptr() for d in d1])
    rng = np.random.default_rng(5)
    kps, is3, sid = [], [], []
    for s in range(S):
        k = orc.detect(streams[s][0][0], np.zeros((0, 2)), max_points=60 + 20 * s).astype(float)
        k = np.concatenate([k, np.array([[1.0, 1.0], [H, W], [2.5, W - 1.5]])])
        kps.append(k); is3.append(rng.random(len(k)) < 0.5); sid.append(np.full(len(k), s, np.int32))
    shift = np.array([streams[s][2][1] for s in range(S)], dtype=np.float64)
    shift[2] += (0.0, 40.0)
    P, T, I = np.concatenate(kps), np.concatenate(is3), np.concatenate(sid)
    proj = P + shift[I]
    inside = (proj[:, 0] >= 1) & (proj[:, 0] <= H) & (proj[:, 1] >= 1) & (proj[:, 1] <= W)
    return dict(a=a, b=b, kps=kps, is3=is3, shift=shift, P=P, T=T, I=I, proj=proj, skip=T & ~inside, keep=(d0, d1))


@pytest.mark.parametrize("window", [7, 10])
def test_every_seam_gives_the_same_tracks(slam, syn, scene, window):
    """windows 7 and 10: the first on the 6-slot and on the 9-slot kernels.  Positions (NaN where lost), status (0 lost, 1 tracked, 2 skipped:
    a 3-D keypoint projected outside the image) and kept indices of (i) the device-resident set, (ii) the kept-list batch seam, (iii) the
    fused per-stream seam and (iv) the reference's two fb_tracking! calls are equal in every bit."""
    a, b, P, T, I, proj, skip = (scene[k] for k in ("a", "b", "P", "T", "I", "proj", "skip"))
    params = slam.Params(stereo=True, max_nb_keypoints=150, window_size=window)
    n = len(P)
    ns = np.flatnonzero(~skip)

    def result(tracked_idx, tracked_pos):
        pos = np.full((n, 2), np.nan); st = np.zeros(n, np.uint8)
        pos[tracked_idx] = tracked_pos; st[tracked_idx] = 1
        pos[skip] = P[skip]; st[skip] = 2
        return pos, st

    # (i) the set: ids carry the input index through the compaction
    ks = slam.KeypointSet(S, 128)
    for s in range(S):
        ks.upload(s, scene["kps"][s], scene["is3"][s], ids=np.flatnonzero(I == s))
    ks.flow_match(a, b, params, slam.stream_params(S, cam=syn.KITTI_CAM, shift_yx=scene["shift"]), prior=2)
    cnt = ks.counts()
    got = [ks.download(s) for s in range(S)]
    assert [len(g["yx"]) for g in got] == list(cnt)
    kept_i = np.concatenate([g["ids"] for g in got]).astype(np.int64)
    pos_i = np.full((n, 2), np.nan); st_i = np.zeros(n, np.uint8)
    pos_i[kept_i] = np.concatenate([g["yx"] for g in got]); st_i[kept_i] = np.where(skip[kept_i], 2, 1)
    assert np.array_equal(np.concatenate([g["is_3d"] for g in got]), T[kept_i])
    # (ii) kept-list batch seam
    hk, h3, hs, hsrc = slam.optical_flow_matching_batch_kept(a, b, I[~skip], P[~skip], T[~skip], proj[~skip], params)
    pos_ii, st_ii = result(ns[hsrc], hk)
    assert np.array_equal(h3, T[ns[hsrc]]) and np.array_equal(hs, I[ns[hsrc]])
    # (iii) fused and (iv) two-call per-stream seams
    per = {}
    for fused in (True, False):
        idx, new = [], []
        for s in range(S):
            sel = np.flatnonzero((I == s) & ~skip)
            out, st = slam.optical_flow_matching(a.pyramids[s], b.pyramids[s], P[sel], T[sel], proj[sel], params, fused=fused)
            idx.append(sel[st]); new.append(out[st])
        per[fused] = result(np.concatenate(idx), np.concatenate(new))
    for name, (pos, st) in (("batch_kept", (pos_ii, st_ii)), ("fused", per[True]), ("two calls", per[False])):
        print(window, name, "tracked", int((st == 1).sum()), "lost", int((st == 0).sum()), "skipped", int((st == 2).sum()))
        assert np.array_equal(st, st_i), name
        assert np.array_equal(pos, pos_i, equal_nan=True), name
        assert np.array_equal(np.flatnonzero(st), np.sort(kept_i)), name                       # kept indices
    assert all(np.array_equal(g["ids"], np.sort(g["ids"])) for g in got)                       # the compaction is stable
    # precondition: the second attempt really runs, and every stream loses something
    t2 = np.flatnonzero((I == 2) & T & ~skip)
    _, st_prior = slam.fb_tracking_(a.pyramids[2], b.pyramids[2], P[t2], displacement=0.5 * (proj[t2] - P[t2]), pyramid_levels=1,
                                    window_size=window, max_distance=params.max_ktl_distance)
    lost_prior = t2[~st_prior]
    print(window, "stream 2: prior alone loses", len(lost_prior), "of", len(t2), "3-D keypoints;", int((st_i[lost_prior] == 1).sum()), "of them tracked in the end")
    assert len(lost_prior) >= 5 and (st_i[lost_prior] == 1).sum() >= 3
    assert all(((st_i == 0) & (I == s)).sum() >= 1 for s in range(S))


def test_the_match_seams_refuse_alike(slam, orc, texture):
    """64 x 64 pyramids: every entry point refuses (a) one level too few with the reference's error, (b) a target of another level-0 shape
    with SLAM_ERR_ARG, (c) a source built with target_only=True naming the flag, (d) too few layers AND another shape with the layers
    error (the order of the checks); (e) after each refusal the same context gives the result it gave before.  Every refusal returns
    before anything is launched."""
    import torch
    h = w = 64
    Sb = 2
    streams = [texture(h, w, seed=40 + s, step=(1.1, -0.9), disparity=3.0) for s in range(Sb)]
    d0 = [torch.from_numpy(np.ascontiguousarray(st[0][0].T)).cuda() for st in streams]
    d1 = [torch.from_numpy(np.ascontiguousarray(st[0][1].T)).cuda() for st in streams]
    torch.cuda.synchronize()
    mk = lambda shape=(h, w): slam.PyramidBatch(shape, levels=3, S=Sb)
    A, B, At, Bx = mk(), mk(), mk(), mk((h, w + 2))
    A.update_([d.data_ptr() for d in d0]); B.update_([d.data_ptr() for d in d1]); At.update_([d.data_ptr() for d in d0], target_only=True)
    kp = [orc.detect(streams[s][0][0], np.zeros((0, 2)), max_points=20 + 5 * s).astype(float) for s in range(Sb)]
    assert all(len(k) >= 5 for k in kp)
    rng = np.random.default_rng(2)
    is3 = [rng.random(len(k)) < 0.5 for k in kp]
    flow = np.array([streams[s][2][1] for s in range(Sb)], dtype=np.float64)
    P, T, I = np.concatenate(kp), np.concatenate(is3), np.concatenate([np.full(len(k), s, np.int32) for s, k in enumerate(kp)])
    proj = P + flow[I]
    assert slam.fb_tracking_(A.pyramids[0], B.pyramids[0], kp[0], window_size=9)[1].any()          # the valid match tracks something
    sp = slam.stream_params(Sb, shift_yx=flow)

    def set_call(method, frm, to, params):
        ks = slam.KeypointSet(Sb, 64)
        for s in range(Sb):
            ks.upload(s, kp[s], is3[s])
        getattr(ks, method)(frm, to, params, sp, prior=2)
        got = [ks.download(s) for s in range(Sb)]
        return [g[k] for g in got for k in ("yx", "is_3d", "stereo_yx", "has_stereo")]

    seams = {
        "fb_tracking_": lambda f, t, p: slam.fb_tracking_(f.pyramids[0], t.pyramids[0], kp[0], window_size=p.window_size, pyramid_levels=p.pyramid_levels),
        "optical_flow_matching": lambda f, t, p: slam.optical_flow_matching(f.pyramids[0], t.pyramids[0], kp[0], is3[0], kp[0] + flow[0], p),
        "optical_flow_matching_batch": lambda f, t, p: slam.optical_flow_matching_batch(f, t, I, P, T, proj, p),
        "optical_flow_matching_batch_kept": lambda f, t, p: slam.optical_flow_matching_batch_kept(f, t, I, P, T, proj, p),
        "KeypointSet.flow_match": lambda f, t, p: set_call("flow_match", f, t, p),
        "KeypointSet.stereo_match": lambda f, t, p: set_call("stereo_match", f, t, p),
    }
    ok = slam.Params(stereo=True)
    few = slam.Params(stereo=True, pyramid_levels=A.pyramids[0].levels)          # needs one layer more than the pyramids have
    assert ok.pyramid_levels == A.pyramids[0].levels - 1
    same = lambda x, y: len(x) == len(y) and all(np.array_equal(u, v, equal_nan=True) for u, v in zip(x, y))
    for name, call in seams.items():
        before = call(A, B, ok)
        for what, (frm, to, params, match) in dict(
                a=(A, B, few, r"^Not enough layers in pyramids\.$"), b=(A, Bx, ok, r"libslamhip error -1:"),
                c=(At, B, ok, r"libslamhip error -1:.*TARGET_ONLY"), d=(A, Bx, few, r"^Not enough layers in pyramids\.$")).items():
            with pytest.raises(RuntimeError, match=match):
                call(frm, to, params)
            assert same(call(A, B, ok), before), (name, what)                    # (e)
