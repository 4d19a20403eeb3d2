"""GPU: examples/device_frontend.py run(..., local_ba=True, local_map_match=True, descriptor_rows=4) at 4 streams and 10 key-frames -- the run of
tests/test_gpu_device_frontend_lmm.py on a map that keeps one descriptor row per key-frame and point (KeyframeMap.enable_descriptor_rows).

The run is replayed through the row model (tests/np_kfmap_rows.py) from what the device itself held (run()'s map_probe).  On the example's rigid scene
no pair occurs, so what is compared at every key-frame is the row store of every stream (KeyframeMap.descriptor_rows: ids, the "described" byte, keys
and rows, the dropped counter), the staged local map and keypoint list, and the status -- with the rows following the local BA's outlier removals, the
gather's demotions and the points it removes.  A key-frame's angles are the device's own (1e-12, then its bits are the model's)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_kfmap as npk  # noqa: E402
import np_kfmap_rows as nr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N_FRAMES, KF_EVERY, MAXKP, ROWS = 4, 19, 2, 200, 4
ANGLE_TOL = 1e-12


def _example():
    spec = importlib.util.spec_from_file_location("device_frontend", os.path.join(ROOT, "examples", "device_frontend.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_with_descriptor_rows_equals_the_model(slam, syn):
    ex = _example()
    cam = syn.KITTI_CAM
    H, W = 200, 320
    lefts, rights, offs = ex.synthetic_scene(S, N_FRAMES, shape=(H, W), disparity=8.0, seed=5)
    params = slam.Params()
    cam10 = tuple(cam) + (0.0, 0.0, 0.0, 0.0, float(H), float(W))
    cell = slam.Extractor.from_params(slam.Params(stereo=True, max_nb_keypoints=MAXKP), slam.Camera(*cam, height=H, width=W)).cell_size
    st = dict(m=None, D=None, wm=[None] * S, nkf=[0] * S, n_cmp=0, n_rows=0, n_local=0, n_lost=0, km=None)

    def rows_equal(km, where):
        for s in range(S):
            want = nr.descriptor_rows(st["m"][s], st["D"][s])
            assert nr.same_rows(km.descriptor_rows(s), want), (where, s)
            st["n_rows"] += sum(len(k) for k in want["keys"])
            st["n_lost"] += int(np.sum(want["described"] & (np.array([len(k) for k in want["keys"]]) == 0)))

    def probe(i, stage, *a):
        if stage == "lists":
            ks, kf_mask, Tcw = a
            assert kf_mask.all()
            if st["m"] is None:
                st["m"] = [npk.Map(ks.cap, 16, 8192, cam, None, params.min_cov_score) for _ in range(S)]
                st["D"] = [nr.new_descriptors(m, ROWS) for m in st["m"]]
            elif st["km"] is not None:
                rows_equal(st["km"], ("after the update", i))    # the store as the last key-frame's local BA left it
            for s in range(S):
                nr.add_keyframe(st["m"][s], st["D"][s], st["nkf"][s], Tcw[s], ks.download(s))
                st["nkf"][s] += 1
        elif stage == "added":
            km, = a
            st["km"] = km
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
                nr.add_descriptors(st["m"][s], st["D"][s], int(inf[s, 0]), rows[s, :n])
        elif stage == "matched":
            km, status, pairs, dist = a
            rows_equal(km, ("matched", i))
            for s in range(S):
                w = nr.local_map_match(st["m"][s], st["D"][s], cam10, cell, params, max_local=10 * MAXKP)
                assert w["margin"] >= 1e-9, (i, s, w["margin"])
                assert status[s] == w["status"], (i, s)
                assert np.array_equal(pairs[s], w["pairs"]) and np.array_equal(dist[s], w["dist"]), (i, s)
                d = km.debug_local_map(s)
                assert np.array_equal(d["lm_ids"], w["lm_ids"]) and np.array_equal(d["kp_ids"], w["kp_ids"]), (i, s)
                st["n_cmp"] += 1; st["n_local"] += len(w["lm_ids"])
            st["wm"] = [nr.gather(m, D) for m, D in zip(st["m"], st["D"])]
        elif stage == "solved":
            wins, = a
            for w in wins:
                wm = st["wm"][w.stream]
                assert wm is not None and np.array_equal(w.points_remap, wm["points_remap"]) and np.array_equal(w.obs_kp, wm["obs_kp"])
                nr.update(st["m"][w.stream], st["D"][w.stream], wm, w.cache.theta, w.cache.outliers)

    out, n3 = ex.run(lefts, rights, cam, 0.54, kf_every=KF_EVERY, max_keypoints=MAXKP, seed=9, local_ba=True, local_map_match=True, descriptor_rows=ROWS,
                     map_probe=probe)
    n_kf = (N_FRAMES + KF_EVERY - 1) // KF_EVERY
    assert st["nkf"] == [n_kf] * S and st["n_cmp"] == n_kf * S
    print(f"descriptor rows in the example: {st['n_rows']} rows compared, {st['n_local']} local-map points staged, {st['n_lost']} described points without a row met")
    assert st["n_rows"] > 0 and st["n_local"] > 0
    with pytest.raises(ValueError):
        ex.run(lefts, rights, cam, 0.54, local_ba=True, descriptor_rows=ROWS)
