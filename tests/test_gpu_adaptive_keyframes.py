"""GPU: examples/device_frontend.py with adaptive key-frames -- after the pose of every frame the statistics of the device-resident lists
(KeypointSet.frame_stats) go through keyframe_required (check_new_kf_required, front_end.jl:361-393), and a key-frame is taken for all
lock-stepped streams when any stream requires one.  Every decision is compared with the numpy model (tests/np_kf.py) on the lists downloaded
at that very point; the fixed-period mode must be what it was."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_kf  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N_FRAMES, SHAPE, DISPARITY, BASELINE, MAXKP = 2, 10, (200, 320), 8.0, 0.54, 300


def _example():
    spec = importlib.util.spec_from_file_location("device_frontend", os.path.join(ROOT, "examples", "device_frontend.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def scene(slam, syn):
    ex = _example()
    lefts, rights, offs = ex.synthetic_scene(S, N_FRAMES, shape=SHAPE, disparity=DISPARITY, seed=21)
    return ex, lefts, rights, offs


def test_adaptive_keyframes_follow_the_model(slam, syn, scene):
    ex, lefts, rights, offs = scene
    cam = syn.KITTI_CAM
    lists = {}

    def probe(i, ks, R):                                         # the lists the decision of frame i was taken on
        lists[i] = [(ks.download(s), ks.download_keyframe(s), R[s]) for s in range(S)]

    out, n3 = ex.run(lefts, rights, cam, BASELINE, max_keypoints=MAXKP, seed=9, adaptive=True, probe=probe)
    kf = [r["keyframe"] for r in out]
    print("key-frames:", kf, "rules:", [r.get("kf_rule", np.zeros(0)).tolist() for r in out])
    assert kf[0] and "kf_required" not in out[0]
    assert any(kf[1:]) and not all(kf), kf
    last, prev3d = 0, None
    for i, r in enumerate(out[1:], start=1):
        assert sorted(lists) == list(range(1, N_FRAMES)) and r["frames_delta"].tolist() == [i - last] * S
        for s in range(S):
            d, (kyx, haskf), R = lists[i][s]
            want = np_kf.frame_stats(cam, (0.0, 0.0, 0.0, 0.0), d["yx"], d["is_3d"], d["has_stereo"], kyx, haskf, 1, 35, SHAPE[0], SHAPE[1], R)
            got = r["kf_stats"][s]
            assert np.array_equal(got[:6], want[:6]) and np.abs(got[6:] - want[6:]).max() <= 1e-9, (i, s, got, want)
            req, rule, margin = np_kf.decide(want, i - last, int(r["prev_kf_nb_3d"][s]), True, MAXKP, 20.0, False)
            assert margin >= 1e-6, (i, s, margin, want)          # the model is not on a threshold, so the device's last bits cannot decide
            assert (bool(r["kf_required"][s]), int(r["kf_rule"][s])) == (req, rule), (i, s, r["kf_required"], r["kf_rule"], req, rule, want)
        assert r["keyframe"] == bool(r["kf_required"].any())     # the lock-step policy: any stream's need
        if prev3d is not None:
            assert np.array_equal(r["prev_kf_nb_3d"], prev3d)    # unchanged between key-frames
        prev3d = r["prev_kf_nb_3d"]
        if r["keyframe"]:
            last, prev3d = i, None
    assert out[1]["prev_kf_nb_3d"].min() > 0                     # frame 0's stereo triangulations were counted
    assert any(r["kf_stats"][:, 2].max() > 0 for r in out[1:])   # nb_stereo_kpts: lists that went through the stereo match
    # the motion is still recovered: the 5 cm of the fixed-period test
    Z = cam[0] * BASELINE / DISPARITY
    for s in range(S):
        o = offs[s][-1] - offs[s][0]
        want = np.array([o[1] * Z / cam[0], o[0] * Z / cam[1], 0.0])
        T = out[-1]["poses"][s]
        assert np.abs(T[:3, 3] - want).max() < 0.03 * max(1.0, np.abs(want).max()) + 0.02, (s, T[:3, 3], want)


def test_fixed_period_mode_is_unchanged(slam, syn, scene):
    """adaptive=False: the rows of a run are those of a second run with the same seed, key-frames every 4th frame, and carry no decision fields"""
    ex, lefts, rights, offs = scene
    a, n3a = ex.run(lefts, rights, syn.KITTI_CAM, BASELINE, kf_every=4, max_keypoints=MAXKP, seed=9)
    b, n3b = ex.run(lefts, rights, syn.KITTI_CAM, BASELINE, kf_every=4, max_keypoints=MAXKP, seed=9, adaptive=False)
    assert [r["keyframe"] for r in a] == [i % 4 == 0 for i in range(N_FRAMES)] and n3a == n3b
    for ra, rb in zip(a, b):
        assert set(ra) == {"frame", "keyframe", "poses", "status", "status_5pt", "counts", "ms"} == set(rb)
        for k in ("frame", "keyframe"):
            assert ra[k] == rb[k]
        for k in ("poses", "status", "status_5pt", "counts"):
            assert np.array_equal(ra[k], rb[k]), (ra["frame"], k)
