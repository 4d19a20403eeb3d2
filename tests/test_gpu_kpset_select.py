"""GPU: per-stream key-frames -- slam_kpset_select names the streams the six key-frame seams act on (detect, detect_describe, keyframe,
stereo_match, triangulate, triangulate_temporal).  A selected stream must come out exactly as it does without a selection, an unselected one
exactly as it went in, in every field the three downloads show (download, download_first with the key-frame counter, download_keyframe),
compared byte for byte; the every-frame seams must not see the selection at all.  Shapes and list preparation are test_gpu_kpset.py's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_kpset import _setup  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("yx", "is_3d", "xyz", "ids", "stereo_yx", "has_stereo", "first_yx", "first_kf", "kyx", "has_kf")
T21 = np.eye(4); T21[0, 3] = -0.54                                   # right camera 0.54 m to the right of the left one
TWC = np.eye(4); TWC[:3, 3] = [1.0, 2.0, 3.0]
WINDOW, WORDS = 9, 4


def _snap(ks, s):
    """every field of stream s the host can see"""
    d = ks.download(s)
    f, k, kc = ks.download_first(s)
    kyx, hk = ks.download_keyframe(s)
    d.update(first_yx=f, first_kf=k, kyx=kyx, has_kf=hk, kf_count=kc)
    return d


def _diff(a, b):
    """names of the fields in which two snapshots differ, byte for byte"""
    bad = [k for k in FIELDS if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    return bad + (["kf_count"] if a["kf_count"] != b["kf_count"] else [])


class _Case:
    """S streams at H x W with lists as test_keyframe_step_equals_host_protocol prepares them: ragged counts, some 3-D, border points, one
    key-frame behind them (so the first / key-frame observations are not empty) and one flow_match, so that st holds real statuses (lost
    keypoints 0, 3-D keypoints projected outside 2).  new_set() gives a set in exactly that state, every time."""

    def __init__(self, slam, orc, syn, texture, S, H, W, max_kp, n_of):
        self.slam, self.syn, self.S, self.H, self.W = slam, syn, S, H, W
        self.streams, self.a, self.b, self.r, self.keep = _setup(slam, texture, S, H, W)
        self.params = slam.Params(stereo=True, max_nb_keypoints=max_kp)
        cam = slam.Camera(*syn.KITTI_CAM, height=H, width=W)
        self.e = slam.Extractor.from_params(self.params, cam)
        self.ncell = self.e.grid_resolution[0] * self.e.grid_resolution[1]
        self.cap = max_kp + self.ncell + 8
        self.dcap = self.ncell * -(-max_kp // self.ncell)
        self.pat = slam.brief_pattern(256, WINDOW)
        rng = np.random.default_rng(5)
        self.kps, self.is3 = [], []
        for s in range(S):
            k = orc.detect(np.asfortranarray(self.streams[s][0][0]), np.zeros((0, 2)), max_points=n_of(s)).astype(float)
            k = np.concatenate([k, np.array([[1.0, 1.0], [H, W], [2.5, W - 1.5]])])
            self.kps.append(k); self.is3.append(rng.random(len(k)) < 0.5)
        shift = np.array([self.streams[s][2][1] for s in range(S)])
        self.sp = slam.stream_params(S, cam=syn.KITTI_CAM, shift_yx=shift)
        self.sps = slam.stream_params(S, cam=syn.KITTI_CAM, shift_yx=np.tile([0.0, -6.3], (S, 1)))

    def new_set(self):
        ks = self.slam.KeypointSet(self.S, self.cap)
        for s in range(self.S):
            ks.upload(s, self.kps[s], self.is3[s])
        ks.keyframe()
        ks.flow_match(self.a, self.b, self.params, self.sp, prior=2)
        return ks

    def buffers(self):
        import torch
        desc = torch.full((self.S, self.dcap, WORDS), -7, dtype=torch.int64, device="cuda")
        info = torch.full((self.S, 2), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        return desc, info

    def keyframe_calls(self, ks, desc, info, between=None):
        """one key-frame: detect_describe -> keyframe -> stereo_match -> triangulate; between(): called after the first seam was enqueued"""
        ks.detect_describe(self.e, self.b, desc.data_ptr(), info.data_ptr(), self.dcap, pattern=self.pat, window=WINDOW)
        if between:
            between()
        ks.keyframe()
        ks.stereo_match(self.b, self.r, self.params, self.sps, prior=2)
        ks.triangulate(self.syn.KITTI_CAM, self.syn.KITTI_CAM, T21, TWC, max_error=3.0)

    def results(self, ks, desc, info, streams):
        import torch
        snaps = {s: _snap(ks, s) for s in streams}
        torch.cuda.synchronize()
        return snaps, desc.cpu().numpy(), info.cpu().numpy()


def _check_mask(case, mask, before, ctrl, after_detect, streams):
    """A fresh set with `mask` selected goes through one key-frame: its selected streams equal the control set (no selection), its unselected
    ones their state before; afterwards an unselected detect gives the unselected streams what the same detect gives a set that never had a
    key-frame (after_detect): the lists, ids included -- their id counters were not touched."""
    c_snaps, c_desc, c_info = ctrl
    A = case.new_set()
    m = np.array(mask, dtype=np.uint8)
    from slam_jl_amd import _lib as L
    sent = m.copy()                                                 # through the C entry itself: the wrapper would pass a copy of its own
    A.ctx.check(A.ctx.lib.slam_kpset_select(A.ctx.h, A.h, L.ptr(sent, L.u8p)))
    sent[:] = 1 - sent                                              # the caller's array is free as soon as the call returns
    assert np.array_equal(A.selection(), m.astype(bool))
    desc, info = case.buffers()
    case.keyframe_calls(A, desc, info)
    snaps, d, inf = case.results(A, desc, info, streams)
    for s in streams:
        if m[s]:
            assert _diff(snaps[s], c_snaps[s]) == [], (mask if len(mask) < 8 else "wide", s, "selected stream differs from the control")
            assert tuple(inf[s]) == tuple(c_info[s]) and inf[s, 1] > 0, (s, inf[s], c_info[s])
            n = int(inf[s, 1])
            assert np.array_equal(d[s, :n], c_desc[s, :n]) and (d[s, n:] == -7).all(), s
        else:
            assert _diff(snaps[s], before[s]) == [], (mask if len(mask) < 8 else "wide", s, "unselected stream changed")
            assert inf[s, 0] == c_info[s, 0] and inf[s, 1] == 0, (s, inf[s])       # the id counter (the control's before its append), nothing appended
            assert (d[s] == -7).all(), s                                          # no descriptor row written
    A.select(None)
    A.detect(case.e, case.b)
    for s in streams:
        if not m[s]:
            got = _snap(A, s)
            assert _diff(got, after_detect[s]) == [], (s, "detect after an unselected key-frame")
            assert len(got["ids"]) > len(before[s]["ids"]) and got["ids"][len(before[s]["ids"])] == inf[s, 0], s
    A.close()
    return snaps, d, inf


@pytest.fixture(scope="module")
def small(slam, orc, syn, texture):
    """S = 3 at 120 x 160, 150 keypoints: the prepared state, the control key-frame (no selection) and a plain detect on the prepared state"""
    case = _Case(slam, orc, syn, texture, 3, 120, 160, 150, lambda s: 60 + 20 * s)
    streams = range(3)
    B = case.new_set()
    before = {s: _snap(B, s) for s in streams}
    desc, info = case.buffers()
    case.keyframe_calls(B, desc, info)
    ctrl = case.results(B, desc, info, streams)
    B.close()
    Cs = case.new_set()
    Cs.detect(case.e, case.b)
    after_detect = {s: _snap(Cs, s) for s in streams}
    Cs.close()
    return case, before, ctrl, after_detect


def test_prepared_state_is_worth_the_test(small):
    """ragged lists, 3-D and 2-D keypoints, key-frame observations, and the flow match removed keypoints (statuses 0) and skipped 3-D ones
    projected outside (status 2: [H, W] + shift); the control key-frame appended, matched and triangulated in every stream"""
    case, before, ctrl, _ = small
    lens = [len(before[s]["yx"]) for s in range(3)]
    assert len(set(lens)) == 3 and sum(lens) < sum(len(k) for k in case.kps)      # ragged; the match lost keypoints
    for s in range(3):
        assert before[s]["is_3d"].any() and not before[s]["is_3d"].all() and before[s]["has_kf"].all() and before[s]["kf_count"] == 1
        c = ctrl[0][s]
        assert len(c["yx"]) > lens[s] and c["has_stereo"].sum() > 10 and c["is_3d"].sum() > before[s]["is_3d"].sum() and c["kf_count"] == 2


@pytest.mark.parametrize("mask", [(1, 0, 1), (0, 1, 0), (0, 0, 0), (1, 1, 1)], ids=lambda m: "".join(map(str, m)))
def test_one_keyframe_selected_equals_control_unselected_untouched(small, mask):
    case, before, ctrl, after_detect = small
    _check_mask(case, mask, before, ctrl, after_detect, range(3))


def test_selected_streams_against_the_oracle(small, slam, orc, syn):
    """mask (1, 0, 1): the selected streams' appended keypoints against orc.detect on the stream's own avoidance list (minus the candidates
    describe() drops at the border), the stereo result against optical_flow_matching_frame / triangulate -- the bars of
    test_keyframe_step_equals_host_protocol (positions untouched, map points within 1e-9)."""
    case, before, ctrl, after_detect = small
    H, W, lim = case.H, case.W, (WINDOW + 1) // 2
    A = case.new_set()
    A.select([1, 0, 1])
    desc, info = case.buffers()
    A.detect_describe(case.e, case.b, desc.data_ptr(), info.data_ptr(), case.dcap, pattern=case.pat, window=WINDOW)
    lists = {}
    for s in (0, 2):
        cur = before[s]["yx"]
        fresh = orc.detect(np.asfortranarray(case.streams[s][0][1]), cur, max_points=case.params.max_nb_keypoints)
        inbox = (fresh[:, 0] - lim >= 1) & (fresh[:, 0] + lim <= H) & (fresh[:, 1] - lim >= 1) & (fresh[:, 1] + lim <= W)
        got = A.download(s)
        assert inbox.any() and np.array_equal(got["yx"], np.concatenate([cur, fresh[inbox].astype(float)])), s
        assert np.array_equal(got["is_3d"], np.concatenate([before[s]["is_3d"], np.zeros(int(inbox.sum()), bool)])), s
        lists[s] = (got["yx"], got["is_3d"])
    assert np.array_equal(A.download(1)["yx"], before[1]["yx"])
    A.keyframe()
    A.stereo_match(case.b, case.r, case.params, case.sps, prior=2)
    for s in (0, 2):
        kp, t3 = lists[s]
        res = slam.optical_flow_matching_frame(case.b.pyramids[s], case.r.pyramids[s], kp, t3, kp + np.array([0.0, -6.3]), case.params, (H, W), stereo=True,
                                               undistorted_left=kp, right_cam=syn.KITTI_CAM)
        got = A.download(s)
        keep_s = ~res["removed"]
        assert np.array_equal(got["yx"], kp[keep_s]), s                          # positions untouched, out-of-image 3-D observations removed
        assert np.array_equal(got["has_stereo"], res["updated"][keep_s]), s
        up = got["has_stereo"]
        assert np.array_equal(got["stereo_yx"][up], res["new_pixels"][keep_s][up]) and up.mean() > 0.3, s
        lists[s] = (kp[keep_s], t3[keep_s], got["stereo_yx"], up)
    A.triangulate(syn.KITTI_CAM, syn.KITTI_CAM, T21, TWC, max_error=3.0)
    for s in (0, 2):
        kp, t3, syx, up = lists[s]
        got = A.download(s)
        cand = up & ~t3
        xyz, ok = slam.triangulate(syn.KITTI_CAM, syn.KITTI_CAM, T21, kp[cand], syx[cand], 3.0)
        exp3 = t3.copy(); exp3[np.flatnonzero(cand)[ok]] = True
        exps = up.copy(); exps[np.flatnonzero(cand)[~ok]] = False
        assert np.array_equal(got["is_3d"], exp3) and np.array_equal(got["has_stereo"], exps) and ok.any(), s
        world = xyz[ok] + TWC[:3, 3]
        assert np.abs(got["xyz"][np.flatnonzero(cand)[ok]] - world).max() <= 1e-9 * max(1.0, np.abs(world).max()), s
    assert _diff(_snap(A, 1), before[1]) == []
    A.close()


SCHEDULES = ({0, 2, 4, 6}, {0, 3}, {0, 5})                           # the frames at which stream 0 / 1 / 2 takes a key-frame
N_FRAMES, NKF = 7, 4


def _kf_pose(k, s):
    """world -> camera of key-frame k of stream s (any rigid motion will do: the seam under test only has to see the same one in both runs)"""
    th = 0.01 * k
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    T[:3, 3] = [-0.6 * k - 0.1 * s, 0.02 * k, -0.3 * k]
    return T


def _run_schedules(slam, syn, seq, schedules, use_select):
    """7 frames on S = 3 streams: flow_match every frame; where a stream's schedule says key-frame: remove (cull flags zero for the others),
    detect, keyframe, stereo_match, triangulate, triangulate_temporal with per-stream kf_cur.  use_select: the key-frame seams run under
    select(mask of the frame); else no selection is ever set (then all schedules are one schedule).  Returns snapshots [frame][stream]."""
    import torch
    lefts, rights, params, e, cap, shift = seq
    S = 3
    ks = slam.KeypointSet(S, cap)
    n_kf = np.zeros(S, np.int32)
    kf_cw = np.tile(np.eye(4), (S, NKF, 1, 1))
    sp_flow = slam.stream_params(S, cam=syn.KITTI_CAM, shift_yx=shift)
    sps = slam.stream_params(S, cam=syn.KITTI_CAM, shift_yx=np.tile([0.0, -6.3], (S, 1)))
    out, temporal_changed = [], False
    for f in range(N_FRAMES):
        if f > 0:
            ks.flow_match(lefts[f - 1], lefts[f], params, sp_flow, prior=2)
        mask = np.array([f in schedules[s] for s in range(S)])
        if not use_select:
            assert mask.all() or not mask.any()
        if mask.any():
            flags = np.zeros((S, cap), np.uint8)
            for s in np.flatnonzero(mask):
                flags[s] = np.random.default_rng(1000 * f + s).random(cap) < 0.15          # the stream's cull of this frame, whoever else culls
            fdev = torch.from_numpy(flags).cuda(); torch.cuda.synchronize()
            ks.remove(fdev.data_ptr())
        if use_select:
            ks.select(mask)
        if mask.any() or use_select:                                 # (under a selection the seams are also called with no stream selected)
            ks.detect(e, lefts[f])
            ks.keyframe()
            ks.stereo_match(lefts[f], rights[f], params, sps, prior=2)
            ks.triangulate(syn.KITTI_CAM, syn.KITTI_CAM, T21, TWC, max_error=3.0)
            kf_cur = np.where(mask, n_kf, -12345).astype(np.int32)   # an unselected stream's kf_cur / table / pose rows are never read
            Twc = np.zeros((S, 4, 4))
            for s in np.flatnonzero(mask):
                kf_cw[s, n_kf[s] % NKF] = _kf_pose(n_kf[s], s)
                Twc[s] = np.linalg.inv(_kf_pose(n_kf[s] + 0.4, s))
            for s in np.flatnonzero(~mask):
                Twc[s] = np.eye(4)
            pre = [_snap(ks, s) for s in range(S)] if not use_select else None
            ks.triangulate_temporal(slam.stream_params(S, cam=syn.KITTI_CAM), kf_cw, Twc, kf_cur, max_error=3.0)
            if pre is not None:
                temporal_changed |= any(_diff(_snap(ks, s), pre[s]) != [] for s in range(S))
            n_kf[mask] += 1
        out.append([_snap(ks, s) for s in range(S)])
    ks.close()
    return out, temporal_changed


def test_per_stream_schedules_over_seven_frames(slam, syn, texture):
    """Stream s of the run with per-frame selections equals stream s of a run without any selection in which all streams follow s's
    schedule, in every field after every frame (today's seams never let one stream's output depend on another's: test_gpu_work_order.py
    and the kpset tests pin that).  The schedules give frames with none, one and all streams selected; the mono path (triangulate_temporal,
    with its compaction) runs at every key-frame."""
    import torch
    S, H, W = 3, 120, 160
    streams = [texture(H, W, n=N_FRAMES, seed=30 + s, step=(1.0 + 0.2 * s, -1.4), disparity=6.3) for s in range(S)]
    params = slam.Params(stereo=True, max_nb_keypoints=150)
    e = slam.Extractor.from_params(params, slam.Camera(*syn.KITTI_CAM, height=H, width=W))
    cap = params.max_nb_keypoints + e.grid_resolution[0] * e.grid_resolution[1] + 8
    keep, lefts, rights = [], [], []
    for f in range(N_FRAMES):
        for side, dst in ((0, lefts), (1, rights)):
            d = [torch.from_numpy(np.ascontiguousarray(st[side][f].T)).cuda() for st in streams]
            torch.cuda.synchronize()
            pb = slam.PyramidBatch((H, W), levels=3, S=S)
            pb.update_([t.data_ptr() for t in d])
            keep.append(d); dst.append(pb)
    shift = np.array([[streams[s][2][1][0] - streams[s][2][0][0], streams[s][2][1][1] - streams[s][2][0][1]] for s in range(S)])
    seq = (lefts, rights, params, e, cap, shift)
    n_sel = [sum(f in SCHEDULES[s] for s in range(S)) for f in range(N_FRAMES)]
    assert {0, 1, 3} <= set(n_sel)                                   # frames with none, one and all streams selected
    got, _ = _run_schedules(slam, syn, seq, SCHEDULES, True)
    for s in range(S):
        want, changed = _run_schedules(slam, syn, seq, (SCHEDULES[s],) * S, False)
        assert changed, s                                            # the temporal triangulation did something in the control run
        for f in range(N_FRAMES):
            assert _diff(got[f][s], want[f][s]) == [], (s, f)
        assert want[-1][s]["kf_count"] == len(SCHEDULES[s]) and want[-1][s]["is_3d"].any() and want[-1][s]["has_stereo"].any()
    # the schedules differ, so the streams' lists do: the comparison above could not pass by every run doing the same thing
    assert got[-1][0]["kf_count"] != got[-1][1]["kf_count"]


def test_more_than_64_streams(slam, orc, syn, texture):
    """S = 70 at 96 x 128 (test_gpu_kpset.py's test_more_than_64_streams: the selected work list's offsets and the index table span more than one
    wave's worth of streams): selection {0, 63, 64, 69}, then its complement, one key-frame each; checked on streams on both sides of the
    wave boundary and at both ends."""
    S = 70
    case = _Case(slam, orc, syn, texture, S, 96, 128, 80, lambda s: 30 + (s * 7) % 40)
    check = (0, 1, 62, 63, 64, 65, 69)
    B = case.new_set()
    before = {s: _snap(B, s) for s in check}
    desc, info = case.buffers()
    case.keyframe_calls(B, desc, info)
    ctrl = case.results(B, desc, info, check)
    B.close()
    Cs = case.new_set()
    Cs.detect(case.e, case.b)
    after_detect = {s: _snap(Cs, s) for s in check}
    Cs.close()
    mask = np.zeros(S, np.uint8); mask[[0, 63, 64, 69]] = 1
    _check_mask(case, mask, before, ctrl, after_detect, check)
    _check_mask(case, 1 - mask, before, ctrl, after_detect, check)


def test_every_frame_seams_ignore_the_selection(small, slam, syn):
    """with (1, 0, 1) active, flow_match, remove, frame_stats, counts and upload / download do what they do on a set without a selection"""
    import torch
    case, before, _, _ = small
    A, B = case.new_set(), case.new_set()
    A.select([1, 0, 1])
    rng = np.random.default_rng(11)
    flags = (rng.random((case.S, case.cap)) < 0.3).astype(np.uint8)
    fdev = torch.from_numpy(flags).cuda(); torch.cuda.synchronize()
    sp = slam.stream_params(case.S, cam=syn.KITTI_CAM)
    for ks in (A, B):
        ks.remove(fdev.data_ptr())
    for s in range(case.S):
        a, b = _snap(A, s), _snap(B, s)
        assert _diff(a, b) == [] and len(a["yx"]) < len(before[s]["yx"]), s       # stream 1 was culled too
    for ks in (A, B):
        ks.flow_match(case.b, case.a, case.params, slam.stream_params(case.S, cam=syn.KITTI_CAM, shift_yx=-case.sp[:, 24:26]), prior=2)
    assert np.array_equal(A.counts(), B.counts()) and (A.counts() > 0).all()
    sa = A.frame_stats(sp, 1, case.e.cell_size, (case.H, case.W)); sb = B.frame_stats(sp, 1, case.e.cell_size, (case.H, case.W))
    assert sa.tobytes() == sb.tobytes() and (sa[:, 0] == A.counts()).all()
    for s in range(case.S):
        assert _diff(_snap(A, s), _snap(B, s)) == [], s
    for ks in (A, B):                                                # upload replaces the unselected stream's list as any other's
        ks.upload(1, case.kps[1][:7], case.is3[1][:7])
    assert _diff(_snap(A, 1), _snap(B, 1)) == [] and len(A.download(1)["yx"]) == 7
    assert np.array_equal(A.selection(), [True, False, True])        # and none of it changed the selection
    A.close(); B.close()


def test_arguments(small, slam):
    from slam_jl_amd import _lib as L
    case, before, ctrl, _ = small
    ks = case.new_set()
    c = ks.ctx
    assert ks.selection().all()                                      # a new set: every stream
    ks.select([0, 1, 0])
    assert np.array_equal(ks.selection(), [False, True, False])
    ks.select(None)
    assert ks.selection().all()
    raw = np.array([0, 200, 7], np.uint8)                            # any non-zero byte selects
    assert c.lib.slam_kpset_select(c.h, ks.h, L.ptr(raw, L.u8p)) == 0
    assert np.array_equal(ks.selection(), [False, True, True])
    with ks.selected([1, 0, 0]):
        assert np.array_equal(ks.selection(), [True, False, False])
        with ks.selected(None):
            assert ks.selection().all()
        assert np.array_equal(ks.selection(), [True, False, False])
    assert np.array_equal(ks.selection(), [False, True, True])       # the context manager restored what was there
    with pytest.raises(ValueError):
        ks.select([1, 0])
    out = np.full(3, 9, np.uint8)
    assert c.lib.slam_kpset_select(None, ks.h, L.ptr(raw, L.u8p)) == -1 and c.lib.slam_kpset_select(c.h, None, L.ptr(raw, L.u8p)) == -1
    assert c.lib.slam_kpset_selection(None, L.ptr(out, L.u8p)) == -1 and c.lib.slam_kpset_selection(ks.h, None) == -1 and (out == 9).all()
    assert np.array_equal(ks.selection(), [False, True, True])       # the refused calls left the selection alone
    # select(None) restores all streams: the key-frame that follows is the control's
    ks.select(None)
    desc, info = case.buffers()
    case.keyframe_calls(ks, desc, info)
    snaps, _, inf = case.results(ks, desc, info, range(3))
    for s in range(3):
        assert _diff(snaps[s], ctrl[0][s]) == [] and tuple(inf[s]) == tuple(ctrl[2][s]), s
    ks.close()
