"""GPU: examples/device_frontend.py run(..., local_ba=True, map_triangulation=True) at S = 2, 12 frames, the example's default image size -- the
key-frame is recorded right behind the stereo triangulation and KeyframeMap.triangulate_temporal(cam, ks=ks) stands where
KeypointSet.triangulate_temporal stood.

The run is replayed through the bounded model (tests/np_kfmap.py + tests/np_kfmap_tri.py) from what the device itself held: run()'s map_probe hands
over the lists before add_keyframe (downloaded here), the call's counts, and the solved windows.  At every ("triangulated", ...) step the counts, the
ring (every key-frame, every point: ids, live bytes, observers, flags) and the live lists (ids, is_3d, length) must equal the model's; an accepted
point's position is held to rtol 1e-9, atol 1e-9 (numpy against the device's sin / cos and DLT), then the device's bits are the model's.  The gate
quantities of the run's candidates must lie 1e-6 away from their thresholds (a condition on the scene, asserted).  The recovered motion passes the
example's own bar (tests/test_gpu_device_frontend_ba.py: 0.03 max(1, |expected|) + 0.02 m).

Without the flag the example makes the calls it always made: two runs with the flag off give equal rows, and tests/test_gpu_device_frontend_ba.py holds
that path to its expectations."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_kfmap as npk  # noqa: E402
import np_kfmap_tri as nt  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N_FRAMES = 2, 12
ANGLE_TOL = 1e-12


def _example():
    spec = importlib.util.spec_from_file_location("device_frontend", os.path.join(ROOT, "examples", "device_frontend.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _motion_ok(out, offs, cam, Z):
    for s in range(S):
        o = offs[s][-1] - offs[s][0]
        want = np.array([o[1] * Z / cam[0], o[0] * Z / cam[1], 0.0])
        got = out[-1]["poses"][s][:3, 3]
        assert np.abs(got - want).max() < 0.03 * max(1.0, np.abs(want).max()) + 0.02, (s, got, want)


def test_example_with_map_triangulation_equals_the_model(slam, syn):
    ex = _example()
    cam, disparity = syn.KITTI_CAM, 8.0
    lefts, rights, offs = ex.synthetic_scene(S, N_FRAMES, disparity=disparity)
    params = slam.Params(stereo=True)
    st = dict(m=None, nkf=[0] * S, lst=[None] * S, wm=[None] * S, steps=0, counts=np.zeros(4, dtype=np.int64), ks=None)

    def gather_all():
        for s in range(S):
            st["wm"][s] = npk.gather(st["m"][s])

    def probe(i, stage, *a):
        if stage == "lists":
            ks, kf_mask, Tcw = a
            assert kf_mask.all()
            st["ks"] = ks
            if st["m"] is None:
                st["m"] = [npk.Map(ks.cap, 16, 8192, cam, None, params.min_cov_score) for _ in range(S)]
            for s in range(S):
                st["lst"][s] = ks.download(s)
                npk.add_keyframe(st["m"][s], st["nkf"][s], Tcw[s], st["lst"][s])
                st["nkf"][s] += 1
        elif stage == "added":
            km, = a
            for s in range(S):
                m, k = st["m"][s], st["nkf"][s] - 1
                th, ref = km.download_keyframe(s, k)["theta"], m.theta[k % m.R]
                assert np.array_equal(th[3:], ref[3:]) and np.all(np.abs(th[:3] - ref[:3]) <= ANGLE_TOL), (s, k)
                m.theta[k % m.R] = th
            if st["nkf"][0] == 1:                                # the first key-frame: no triangulation follows, the gather is next
                gather_all()
        elif stage == "triangulated":
            km, counts = a
            for s in range(S):
                m = st["m"][s]
                r = nt.triangulate_temporal(m, cam, st["lst"][s], params.max_reprojection_error, 0.1, 20.0)
                assert np.array_equal(counts[s], r["counts"]), (i, s, counts[s], r["counts"])
                assert all(c["margin"] >= 1e-6 and abs(c["bz"]) >= 0.1 for c in r["cand"]), "the scene puts a gate within 1e-6 of its threshold"
                d = km.download_points(s)
                at = {int(v): j for j, v in enumerate(d["ids"])}
                for c in r["cand"]:
                    if c["code"] == nt.ACCEPTED:                 # the position to its bar, then the device's bits are the model's
                        dev = d["xyz"][at[c["id"]]]
                        assert np.allclose(dev, c["xyz"], rtol=1e-9, atol=1e-9), (i, s, c["id"], np.abs(dev - c["xyz"]).max())
                        m.xyz[c["id"] % m.mcap] = dev
                w = m.points()
                assert all(np.array_equal(d[k], w[k]) for k in ("ids", "xyz", "is_3d", "observed", "ba", "gone")) and d["observers"] == w["observers"], (i, s)
                for kfid in range(st["nkf"][s]):
                    dk, wk = km.download_keyframe(s, kfid), m.keyframe(kfid)
                    assert (dk is None) == (wk is None) and (wk is None or all(np.array_equal(dk[k], wk[k]) for k in ("theta", "ids", "upx", "live"))), (i, s, kfid)
                got = st["ks"].download(s)
                assert len(got["ids"]) == len(r["list"]["ids"]) and np.array_equal(got["ids"], r["list"]["ids"]) and np.array_equal(got["is_3d"], r["list"]["is_3d"]), (i, s)
                st["counts"] += r["counts"]
            st["steps"] += 1
            gather_all()
        elif stage == "solved":
            wins, = a
            assert [w.stream for w in wins] == [s for s in range(S) if st["wm"][s] is not None]
            for w in wins:
                wm = st["wm"][w.stream]
                for a_, b_ in ((w.poses_remap, wm["poses_remap"]), (w.points_remap, wm["points_remap"]), (w.obs_kf, wm["obs_kf"]), (w.obs_kp, wm["obs_kp"])):
                    assert np.array_equal(a_, b_)
                npk.update(st["m"][w.stream], wm, w.cache.theta, w.cache.outliers)

    out, n3 = ex.run(lefts, rights, cam, 0.54, local_ba=True, map_triangulation=True, map_probe=probe)
    n_kf = (N_FRAMES + 3) // 4
    assert st["nkf"] == [n_kf] * S and st["steps"] == n_kf - 1 and sum("tri" in r for r in out) == n_kf - 1
    print(f"temporal triangulation on the map, {st['steps']} steps: candidates, triangulated, removed, skipped = {st['counts'].tolist()}")
    _motion_ok(out, offs, cam, cam[0] * 0.54 / disparity)
    with pytest.raises(ValueError):
        ex.run(lefts, rights, cam, 0.54, map_triangulation=True)


def test_without_the_flag_the_example_is_what_it_was(slam, syn):
    ex = _example()
    cam, disparity = syn.KITTI_CAM, 8.0
    lefts, rights, offs = ex.synthetic_scene(S, N_FRAMES, disparity=disparity)
    stages = [[], []]
    runs = [ex.run(lefts, rights, cam, 0.54, local_ba=True, map_probe=lambda i, stage, *a, k=k: stages[k].append((i, stage)))[0] for k in range(2)]
    assert stages[0] == stages[1] and not any(stage == "triangulated" for _, stage in stages[0])
    kf = [i for i, stage in stages[0] if stage == "lists"]
    assert all(stages[0][j + 1] == (i, "added") for j, (i, stage) in enumerate(stages[0]) if stage == "lists") and kf == [0, 4, 8]
    for ra, rb in zip(*runs):
        assert "tri" not in ra and ra["keyframe"] == rb["keyframe"]
        assert np.array_equal(ra["poses"], rb["poses"]) and np.array_equal(ra["counts"], rb["counts"]) and np.array_equal(ra["status"], rb["status"])
        assert [w[:5] for w in ra.get("ba", [])] == [w[:5] for w in rb.get("ba", [])]
    _motion_ok(runs[0], offs, cam, cam[0] * 0.54 / disparity)
