"""GPU: examples/device_frontend.py run(..., local_ba=True, local_map_match=True, merge=True) against its run without the merge, at 3 streams and 6
key-frames.  On the rigid scene the local-map match finds no pair (a keypoint that is lost is not detected again under a new id), so the flag shows the
wiring -- KeyframeMap.merge(ks) runs behind every match, takes the pairs where the match left them on the device and reports zero counts for every
stream -- and that a call without pairs changes nothing: poses, list lengths, windows and the final map points are those of the run without it."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N_FRAMES, KF_EVERY, MAXKP = 3, 11, 2, 150


def _example():
    spec = importlib.util.spec_from_file_location("device_frontend", os.path.join(ROOT, "examples", "device_frontend.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_with_merge_equals_the_run_without_it(slam, syn):
    ex = _example()
    cam = syn.KITTI_CAM
    lefts, rights, offs = ex.synthetic_scene(S, N_FRAMES, shape=(200, 320), disparity=8.0, seed=5)
    maps = {False: [], True: []}

    def probe_for(flag):
        def probe(i, stage, *a):
            if stage == "solved":                                # behind match (and merge), before the update: the map the estimator reads
                maps[flag].append([(w.stream, w.points_remap.tobytes(), w.obs_kp.tobytes(), w.cache.pixels.tobytes()) for w in a[0]])
        return probe
    runs = {flag: ex.run(lefts, rights, cam, 0.54, kf_every=KF_EVERY, max_keypoints=MAXKP, seed=9, local_ba=True, local_map_match=True, merge=flag,
                         map_probe=probe_for(flag)) for flag in (False, True)}
    (plain, n3_plain), (merged, n3_merged) = runs[False], runs[True]
    n_kf = (N_FRAMES + KF_EVERY - 1) // KF_EVERY
    rows = [r for r in merged if "merged" in r]
    assert len(rows) == n_kf and not any("merged" in r for r in plain)
    for r in rows:                                               # zero pairs on every stream, at every key-frame
        assert r["merged"].shape == (S, 4) and not r["merged"].any()
        assert all(len(p) == 0 for p in r["lmm"][1])
    assert n3_plain == n3_merged and maps[False] == maps[True] and len(maps[True]) >= 2
    for a, b in zip(plain, merged):
        assert np.array_equal(a["poses"], b["poses"]) and np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["status"], b["status"])
        assert a.get("ba") == b.get("ba")
    with pytest.raises(ValueError):
        ex.run(lefts, rights, cam, 0.54, local_ba=True, merge=True)
