"""GPU: examples/device_frontend.py run(..., local_ba=True, local_map_match=True, local_map_history=True) at 4 streams and 10 key-frames, replayed
through the models (tests/np_kfmap.py for the map, tests/np_kfmap_local_map_history.py for the match with its stored local maps) from what the device
itself held, as tests/test_gpu_device_frontend_lmm.py does for the match without history.  At every key-frame the status, the pairs, the staged lists
and the stored set of every key-frame of the ring (KeyframeMap.local_map_ids) must equal the model's.  The rigid scene yields no pairs, as before: a
keypoint that is lost is not detected again under a new id.  Nor does the chain add a point here: with 10 key-frames in a ring of 16 every key-frame
stays covisible with the newest one, so the oldest covisible key-frame's stored set holds nothing the covisibility pass does not give (the count is
printed; the scripted scenes of tests/test_gpu_kfmap_local_map_history.py carry the chain-reached points and pairs).  What the flag shows here is the
wiring: every key-frame's set is stored, and staged lists and stored sets on the device are the model's."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_kfmap as npk  # noqa: E402
import np_kfmap_local_map as nl  # noqa: E402
import np_kfmap_local_map_history as nh  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N_FRAMES, KF_EVERY, MAXKP = 4, 19, 2, 200
R, MCAP = 16, 8192                       # the example's map
ANGLE_TOL = 1e-12


def _example():
    spec = importlib.util.spec_from_file_location("device_frontend", os.path.join(ROOT, "examples", "device_frontend.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_with_local_map_history_equals_the_model(slam, syn):
    ex = _example()
    cam = syn.KITTI_CAM
    H, W = 200, 320
    lefts, rights, offs = ex.synthetic_scene(S, N_FRAMES, shape=(H, W), disparity=8.0, seed=5)
    params = slam.Params()
    cam10 = tuple(cam) + (0.0, 0.0, 0.0, 0.0, float(H), float(W))
    cell = slam.Extractor.from_params(slam.Params(stereo=True, max_nb_keypoints=MAXKP), slam.Camera(*cam, height=H, width=W)).cell_size
    st = dict(m=None, D=None, H=None, wm=[None] * S, nkf=[0] * S, n_cmp=0, n_pairs=0, n_local=0, n_chain=0, n_sets=0)

    def probe(i, stage, *a):
        if stage == "lists":
            ks, kf_mask, Tcw = a
            assert kf_mask.all()
            if st["m"] is None:
                st["m"] = [npk.Map(ks.cap, R, MCAP, cam, None, params.min_cov_score) for _ in range(S)]
                st["D"] = [nl.new_descriptors(m) for m in st["m"]]
                st["H"] = [nh.History(R) for _ in range(S)]
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
                nl.add_descriptors(st["m"][s], st["D"][s], int(inf[s, 0]), rows[s, :int(inf[s, 1])])
        elif stage == "matched":
            km, status, pairs, dist = a
            assert km.mcap == MCAP and km.R == R
            for s in range(S):
                m = st["m"][s]
                w = nh.local_map_match(m, st["D"][s], st["H"][s], cam10, cell, params, max_local=MCAP)
                assert w["margin"] >= 1e-9, (i, s, w["margin"])
                assert status[s] == w["status"] and status[s] != 2, (i, s)
                assert np.array_equal(pairs[s], w["pairs"]) and np.array_equal(dist[s], w["dist"]), (i, s)
                d = km.debug_local_map(s)
                assert np.array_equal(d["lm_ids"], w["lm_ids"]) and np.array_equal(d["kp_ids"], w["kp_ids"]), (i, s)
                for k in range(max(m.cur - R + 1, 0), m.cur + 1):
                    assert np.array_equal(km.local_map_ids(s, k), st["H"][s].ids(m, k)), (i, s, k)
                    st["n_sets"] += 1
                st["n_cmp"] += 1; st["n_pairs"] += len(w["pairs"]); st["n_local"] += len(w["lm_ids"]); st["n_chain"] += len(set(w["lm_ids"]) - set(w["C"]))
            st["wm"] = [npk.gather(m) for m in st["m"]]                # the gather that follows on the device (it demotes is_bad points, window or not)
        elif stage == "solved":
            wins, = a
            for w in wins:
                wm = st["wm"][w.stream]
                assert wm is not None and np.array_equal(w.points_remap, wm["points_remap"]) and np.array_equal(w.obs_kp, wm["obs_kp"])
                npk.update(st["m"][w.stream], wm, w.cache.theta, w.cache.outliers)

    out, n3 = ex.run(lefts, rights, cam, 0.54, kf_every=KF_EVERY, max_keypoints=MAXKP, seed=9, local_ba=True, local_map_match=True, local_map_history=True,
                     map_probe=probe)
    n_kf = (N_FRAMES + KF_EVERY - 1) // KF_EVERY
    assert st["nkf"] == [n_kf] * S and st["n_cmp"] == n_kf * S and st["n_sets"] == S * n_kf * (n_kf + 1) // 2
    print(f"local-map history in the example: {st['n_local']} local-map points staged, {st['n_chain']} of them outside the covisibility pass's, "
          f"{st['n_pairs']} pairs over {n_kf} key-frames")
    assert st["n_local"] > 0
    with pytest.raises(ValueError):
        ex.run(lefts, rights, cam, 0.54, local_ba=True, local_map_history=True)
