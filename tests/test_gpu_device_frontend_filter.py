"""GPU: examples/device_frontend.py run(..., local_ba=True, map_filtering=True) on its smallest scene -- after every key-frame step the map in HBM
is filled from the lists, the windows are gathered, solved and written back, and then KeyframeMap.filter drops the redundant key-frames.

The run is replayed through the bounded model (tests/np_kfmap.py + tests/np_kfmap_filter.py) from what the device itself held: run()'s map_probe
hands over the lists before add_keyframe (downloaded here), the solved windows, and the filter's answer.  The model's add_keyframe / gather /
update / filter_map run on those lists and solutions; the filter's decisions (the removed key-frame ids of every stream at every key-frame) and
the ring's contents (every key-frame so far, every point) must be equal.  A key-frame's angles are the one number the device computes itself:
checked to 1e-12 (tests/test_gpu_kfmap.py's bar), then the device's bits are the model's.

21 key-frames in a ring of 16, filter_from 3: while key-frame 0 is covisible with the newest one the walk breaks at it, so the rule proper is
reached once the ring has forgotten key-frame 0.  Whether this rigid scene produces a removal is reported, not required."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_kfmap as npk  # noqa: E402
import np_kfmap_filter as flt  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N_FRAMES, KF_EVERY, FILTER_FROM, MAXKP = 2, 41, 2, 3, 300
ANGLE_TOL = 1e-12


def _example():
    spec = importlib.util.spec_from_file_location("device_frontend", os.path.join(ROOT, "examples", "device_frontend.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_with_map_filtering_equals_the_model(slam, syn):
    ex = _example()
    cam = syn.KITTI_CAM
    lefts, rights, offs = ex.synthetic_scene(S, N_FRAMES, shape=(200, 320), disparity=8.0, seed=5)
    params = slam.Params()
    st = dict(m=None, nkf=[0] * S, wm=[None] * S, logs=[], n_cmp=0)

    def same_ring(km):
        for s in range(S):
            m = st["m"][s]
            for kfid in range(st["nkf"][s] + 1):
                d, r = km.download_keyframe(s, kfid), m.keyframe(kfid)
                assert (d is None) == (r is None), (s, kfid)
                if r is not None:
                    for k in ("theta", "ids", "upx", "live"):
                        assert np.array_equal(d[k], r[k]), (s, kfid, k)
            d, r = km.download_points(s), m.points()
            assert np.array_equal(d["ids"], r["ids"]) and np.array_equal(d["xyz"], r["xyz"]) and d["observers"] == r["observers"], s
            for k in ("is_3d", "observed", "ba", "gone"):
                assert np.array_equal(d[k], r[k]), (s, k)
            st["n_cmp"] += 1

    def probe(i, stage, *a):
        if stage == "lists":
            ks, kf_mask, Tcw = a
            assert kf_mask.all()
            if st["m"] is None:
                st["m"] = [npk.Map(ks.cap, 16, 8192, cam, None, params.min_cov_score) for _ in range(S)]
            for s in range(S):
                npk.add_keyframe(st["m"][s], st["nkf"][s], Tcw[s], ks.download(s))
                st["nkf"][s] += 1
        elif stage == "added":
            km, = a
            for s in range(S):
                m, k = st["m"][s], st["nkf"][s] - 1
                th, ref = km.download_keyframe(s, k)["theta"], m.theta[k % m.R]
                assert np.array_equal(th[3:], ref[3:]) and np.all(np.abs(th[:3] - ref[:3]) <= ANGLE_TOL), (s, k)
                m.theta[k % m.R] = th
                st["wm"][s] = npk.gather(m)
        elif stage == "solved":
            wins, = a
            assert [w.stream for w in wins] == [s for s in range(S) if st["wm"][s] is not None]
            for w in wins:
                wm = st["wm"][w.stream]
                for a_, b_ in ((w.poses_remap, wm["poses_remap"]), (w.points_remap, wm["points_remap"]), (w.obs_kf, wm["obs_kf"]), (w.obs_kp, wm["obs_kp"]),
                               (w.obs_in_covmap, wm["obs_in_covmap"])):
                    assert np.array_equal(a_, b_)
                npk.update(st["m"][w.stream], wm, w.cache.theta, w.cache.outliers)
        elif stage == "filtered":
            km, removed = a
            logs = [flt.filter_map(st["m"][s], params.filtering_ratio, params.min_cov_score, FILTER_FROM) for s in range(S)]
            st["logs"].append(logs)
            assert removed == [sorted(k for k, e, _, _ in log if e in ("few", "ratio")) for log in logs], (i, removed, logs)      # the decisions
            same_ring(km)                                                                                                        # the ring's contents

    out, n3 = ex.run(lefts, rights, cam, 0.54, kf_every=KF_EVERY, max_keypoints=MAXKP, seed=9, local_ba=True, map_filtering=True, filter_from=FILTER_FROM,
                     map_probe=probe)
    n_kf = (N_FRAMES + KF_EVERY - 1) // KF_EVERY
    assert st["nkf"] == [n_kf] * S and len(st["logs"]) == n_kf and st["n_cmp"] == n_kf * S
    exits = sorted({e for logs in st["logs"] for log in logs for _, e, _, _ in log})
    removed = [sorted(k for r in out for k in r.get("removed", [[]] * S)[s]) for s in range(S)]
    print(f"map filtering on the rigid scene: exits met {exits}, removed key-frames per stream {removed}")
    assert "break" in exits and any(e != "break" for e in exits), exits      # the walk ran both under key-frame 0 and, once the ring forgot it, past it
    assert sum(1 for r in out for w in r.get("ba", [])) >= n_kf              # the local BA kept solving windows beside the filter
    with pytest.raises(ValueError):
        ex.run(lefts, rights, cam, 0.54, map_filtering=True)
