"""GPU: examples/device_frontend.py with per-stream key-frames and COMPACT right builds -- at a key-frame only the right frames of the streams that
asked are uploaded, built (PyramidBatch.update_selected_, into the first members of the right batch) and matched (stereo_match(..., compact=True)).
The rows of such a run -- poses, status words, list lengths, key-frame decisions and the statistics they were taken on -- must be exactly those of
the run that builds the whole right batch at every key-frame (run(..., whole_right_build=True): the behaviour before the compact builds existed),
on test_gpu_per_stream_keyframes.py's three streams, whose key-frame schedules differ.  Once more with right_members=2: the right batch then has two
members for three streams, frame 0 (every stream takes a key-frame) falls back to the whole-batch build, the later key-frames fit."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N_FRAMES, SHAPE, DISPARITY, BASELINE, MAXKP = 3, 10, (200, 320), 8.0, 0.54, 300
STEPS = ((1.1, -1.6), (0.05, -0.05), (3.6, -4.8))
EXACT = ("keyframe", "poses", "status", "status_5pt", "counts", "kf_stats", "kf_required", "kf_rule", "frames_delta", "prev_kf_nb_3d")


def _example():
    spec = importlib.util.spec_from_file_location("device_frontend", os.path.join(ROOT, "examples", "device_frontend.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def scene(slam, syn):
    """the frames, and the rows of the whole-batch run they are all held against"""
    ex = _example()
    lefts, rights = [], []
    for s in range(S):
        L, R, _ = syn.stereo_stream(SHAPE, N_FRAMES, seed=21 + s, step=STEPS[s], disparity=DISPARITY)
        lefts.append(L); rights.append(R)
    run = lambda **kw: ex.run(lefts, rights, syn.KITTI_CAM, BASELINE, max_keypoints=MAXKP, seed=9, per_stream=True, **kw)
    want, n3 = run(whole_right_build=True)
    kf = np.array([r["keyframe"] for r in want])
    assert kf[0].all() and any(0 < kf[i].sum() < S for i in range(1, N_FRAMES)), kf       # frames at which some streams take a key-frame and others do not
    assert len({tuple(np.flatnonzero(kf[:, s])) for s in range(S)}) >= 2, kf                # the schedules differ
    assert all(r["right_build"] == "whole" for r in want if r["keyframe"].any()) and min(n3) > 0
    return run, want, n3, kf


def _same_rows(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for k in EXACT:
            assert (k in g) == (k in w), (i, k)
            if k in w:
                assert np.array_equal(np.asarray(g[k]), np.asarray(w[k])), (i, k, g[k], w[k])


def test_compact_right_builds_give_the_whole_batch_rows(scene):
    run, want, n3, kf = scene
    got, g3 = run()
    _same_rows(got, want)
    assert g3 == n3
    assert [r.get("right_build") for r in got] == ["compact" if kf[i].any() else None for i in range(N_FRAMES)]


def test_two_right_members_for_three_streams(scene):
    run, want, n3, kf = scene
    got, g3 = run(right_members=2)
    _same_rows(got, want)
    assert g3 == n3
    builds = [r.get("right_build") for r in got]
    assert builds[0] == "whole"                                      # three streams asked, the batch holds two
    assert builds == [None if not kf[i].any() else "compact" if kf[i].sum() <= 2 else "whole" for i in range(N_FRAMES)] and "compact" in builds


def test_right_members_needs_per_stream(slam, syn):
    ex = _example()
    L, R, _ = syn.stereo_stream((64, 64), 1, seed=0)
    with pytest.raises(ValueError, match="right_members"):
        ex.run([L], [R], syn.KITTI_CAM, BASELINE, right_members=1)
    with pytest.raises(ValueError, match="right_members"):
        ex.run([L, L], [R, R], syn.KITTI_CAM, BASELINE, per_stream=True, right_members=3)
