"""GPU: examples/device_frontend.py with per-stream key-frames (run(..., per_stream=True)) -- frame 0 is a key-frame for every stream, afterwards
stream s takes a key-frame exactly where keyframe_required (check_new_kf_required, front_end.jl:361-393) says so for s: the key-frame seams run
under KeypointSet.selected(required).  Every decision is compared with the numpy model (tests/np_kf.py) on the lists downloaded at that very
point, as in test_gpu_adaptive_keyframes.py; the streams must end up with DIFFERENT key-frame schedules, and every stream's motion is still
recovered within test_gpu_device_frontend.py's bar.

The streams' motions are chosen so that the schedules differ (the example's default scene moves all streams alike): stream 0 moves as the default
scene's stream 0 (about 1.9 px per frame), stream 1 is nearly stationary (0.07 px per frame: its parallax never reaches the rule's bar, only the rules on counts and cells can ask),
stream 2 moves 6 px per frame (its parallax grows three times as fast as stream 0's).  On an MI355X this gave key-frames at frames {0, 5, 10} for
streams 0 and 1 (the sparse-cells rule) and {0, 4, 8} for stream 2 (the parallax rule)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_kf  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N_FRAMES, SHAPE, DISPARITY, BASELINE, MAXKP = 3, 12, (200, 320), 8.0, 0.54, 300
STEPS = ((1.1, -1.6), (0.05, -0.05), (3.6, -4.8))


def _example():
    spec = importlib.util.spec_from_file_location("device_frontend", os.path.join(ROOT, "examples", "device_frontend.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_per_stream_keyframes_follow_the_model(slam, syn):
    ex = _example()
    cam = syn.KITTI_CAM
    lefts, rights, offs = [], [], []
    for s in range(S):                                           # synthetic_scene's plane, one motion per stream
        L, R, flows = syn.stereo_stream(SHAPE, N_FRAMES, seed=21 + s, step=STEPS[s], disparity=DISPARITY)
        lefts.append(L); rights.append(R); offs.append(np.asarray(flows, dtype=np.float64))
    lists = {}

    def probe(i, ks, R):                                         # the lists the decisions of frame i were taken on
        lists[i] = [(ks.download(s), ks.download_keyframe(s), R[s]) for s in range(S)]

    out, n3 = ex.run(lefts, rights, cam, BASELINE, max_keypoints=MAXKP, seed=9, per_stream=True, probe=probe)
    kf = np.array([np.asarray(r["keyframe"]) for r in out])      # (frames, S)
    print("key-frames per stream:", [np.flatnonzero(kf[:, s]).tolist() for s in range(S)], "rules:", [r.get("kf_rule", np.zeros(0)).tolist() for r in out])
    assert kf.shape == (N_FRAMES, S) and kf.dtype == bool and kf[0].all() and "kf_required" not in out[0]
    last = np.zeros(S, int)
    prev3d = [None] * S
    for i, r in enumerate(out[1:], start=1):
        assert r["frames_delta"].tolist() == (i - last).tolist(), (i, r["frames_delta"], last)
        for s in range(S):
            d, (kyx, haskf), R = lists[i][s]
            want = np_kf.frame_stats(cam, (0.0, 0.0, 0.0, 0.0), d["yx"], d["is_3d"], d["has_stereo"], kyx, haskf, 1, 35, SHAPE[0], SHAPE[1], R)
            got = r["kf_stats"][s]
            assert np.array_equal(got[:6], want[:6]) and np.abs(got[6:] - want[6:]).max() <= 1e-9, (i, s, got, want)
            req, rule, margin = np_kf.decide(want, i - last[s], int(r["prev_kf_nb_3d"][s]), True, MAXKP, 20.0, False)
            assert margin >= 1e-6, (i, s, margin, want)          # the model is not on a threshold, so the device's last bits cannot decide
            assert (bool(r["kf_required"][s]), int(r["kf_rule"][s])) == (req, rule), (i, s, r["kf_required"], r["kf_rule"], req, rule, want)
            assert bool(kf[i, s]) == req, (i, s)                 # the stream's own need, nobody else's
            if prev3d[s] is not None:
                assert r["prev_kf_nb_3d"][s] == prev3d[s], (i, s)   # a stream's figure changes only at its own key-frames
            prev3d[s] = r["prev_kf_nb_3d"][s]
            if kf[i, s]:
                last[s], prev3d[s] = i, None
    assert sorted(lists) == list(range(1, N_FRAMES))
    assert out[1]["prev_kf_nb_3d"].min() > 0                     # frame 0's stereo triangulations were counted, in every stream
    # the point of the feature: the streams do not share a schedule
    schedules = [tuple(np.flatnonzero(kf[:, s])) for s in range(S)]
    assert len(set(schedules)) >= 2, schedules
    assert any(0 < kf[i].sum() < S for i in range(1, N_FRAMES)), schedules      # a frame at which some streams took one and others did not
    # the motion of every stream is still recovered (test_gpu_device_frontend.py's bar)
    Z = cam[0] * BASELINE / DISPARITY
    for i in range(1, N_FRAMES):
        assert out[i]["status"].all(), (i, out[i]["status"])
        for s in range(S):
            o = offs[s][i] - offs[s][0]
            want = np.array([o[1] * Z / cam[0], o[0] * Z / cam[1], 0.0])
            T = out[i]["poses"][s]
            assert np.abs(T[:3, :3] - np.eye(3)).max() < 2e-3, (i, s)
            assert np.abs(T[:3, 3] - want).max() < 0.03 * max(1.0, np.abs(want).max()) + 0.02, (i, s, T[:3, 3], want)
