"""GPU: examples/device_frontend.py run(..., local_ba=True, local_map_match=True) at 4 streams and 10 key-frames -- at every key-frame the new keypoints
are described on the device, their descriptors go into the key-frame map, and the local map of every stream's newest key-frame is staged and matched
in HBM (KeyframeMap.local_map_match) before the local BA.

The run is replayed through the models (tests/np_kfmap.py for the map, tests/np_kfmap_local_map.py for descriptors and match) from what the device
itself held: run()'s map_probe hands over the lists before add_keyframe, the descriptor tensors slam_kpset_detect_describe filled, the match's answer
and the solved windows.  Status, pairs and distances must equal the model's at every key-frame, pair for pair (on calls whose margin is >= 1e-9: the
model says when a decision hangs on the last bits).  A key-frame's angles are the device's own (1e-12, then its bits are the model's, as in
tests/test_gpu_device_frontend_filter.py)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_kfmap as npk  # noqa: E402
import np_kfmap_local_map as nl  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N_FRAMES, KF_EVERY, MAXKP = 4, 19, 2, 200
ANGLE_TOL = 1e-12


def _example():
    spec = importlib.util.spec_from_file_location("device_frontend", os.path.join(ROOT, "examples", "device_frontend.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_with_local_map_match_equals_the_model(slam, syn):
    ex = _example()
    cam = syn.KITTI_CAM
    H, W = 200, 320
    lefts, rights, offs = ex.synthetic_scene(S, N_FRAMES, shape=(H, W), disparity=8.0, seed=5)
    params = slam.Params()
    cam10 = tuple(cam) + (0.0, 0.0, 0.0, 0.0, float(H), float(W))
    cell = slam.Extractor.from_params(slam.Params(stereo=True, max_nb_keypoints=MAXKP), slam.Camera(*cam, height=H, width=W)).cell_size
    st = dict(m=None, D=None, wm=[None] * S, nkf=[0] * S, n_cmp=0, n_pairs=0, n_local=0, n_described=0)

    def probe(i, stage, *a):
        if stage == "lists":
            ks, kf_mask, Tcw = a
            assert kf_mask.all()
            if st["m"] is None:
                st["m"] = [npk.Map(ks.cap, 16, 8192, cam, None, params.min_cov_score) for _ in range(S)]
                st["D"] = [nl.new_descriptors(m) for m in st["m"]]
            for s in range(S):
                nl.add_keyframe(st["m"][s], st["D"][s], st["nkf"][s], Tcw[s], ks.download(s))
                st["nkf"][s] += 1
        elif stage == "added":
            km, = a
            for s in range(S):
                m, k = st["m"][s], st["nkf"][s] - 1
                th, ref = km.download_keyframe(s, k)["theta"], m.theta[k % m.R]
                assert np.array_equal(th[3:], ref[3:]) and np.all(np.abs(th[:3] - ref[:3]) <= ANGLE_TOL), (s, k)
                m.theta[k % m.R] = th
        elif stage == "described":
            desc, info, dcap = a
            rows, inf = desc.cpu().numpy().view(np.uint64), info.cpu().numpy()
            for s in range(S):
                n = int(inf[s, 1])
                assert 0 <= n <= dcap
                nl.add_descriptors(st["m"][s], st["D"][s], int(inf[s, 0]), rows[s, :n])
                st["n_described"] += n
        elif stage == "matched":
            km, status, pairs, dist = a
            for s in range(S):
                w = nl.local_map_match(st["m"][s], st["D"][s], cam10, cell, params, max_local=10 * MAXKP)
                assert w["margin"] >= 1e-9, (i, s, w["margin"])
                assert status[s] == w["status"], (i, s)
                assert np.array_equal(pairs[s], w["pairs"]) and np.array_equal(dist[s], w["dist"]), (i, s)
                d = km.debug_local_map(s)
                assert np.array_equal(d["lm_ids"], w["lm_ids"]) and np.array_equal(d["kp_ids"], w["kp_ids"]), (i, s)
                st["n_cmp"] += 1; st["n_pairs"] += len(w["pairs"]); st["n_local"] += len(w["lm_ids"])
            st["wm"] = [npk.gather(m) for m in st["m"]]                # the gather that follows on the device (it demotes is_bad points, window or not)
        elif stage == "solved":
            wins, = a
            for w in wins:
                wm = st["wm"][w.stream]
                assert wm is not None and np.array_equal(w.points_remap, wm["points_remap"]) and np.array_equal(w.obs_kp, wm["obs_kp"])
                npk.update(st["m"][w.stream], wm, w.cache.theta, w.cache.outliers)

    out, n3 = ex.run(lefts, rights, cam, 0.54, kf_every=KF_EVERY, max_keypoints=MAXKP, seed=9, local_ba=True, local_map_match=True, map_probe=probe)
    n_kf = (N_FRAMES + KF_EVERY - 1) // KF_EVERY
    assert st["nkf"] == [n_kf] * S and st["n_cmp"] == n_kf * S
    assert sum(1 for r in out if "lmm" in r) == n_kf
    print(f"local-map match in the example: {st['n_described']} descriptors stored, {st['n_local']} local-map points staged, {st['n_pairs']} pairs over {n_kf} key-frames")
    assert st["n_described"] > 0 and st["n_local"] > 0
    with pytest.raises(ValueError):
        ex.run(lefts, rights, cam, 0.54, local_map_match=True)
