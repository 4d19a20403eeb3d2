"""GPU: slam_local_map_match / _batch against the Python model of the reference (tests/np_local_map.py: src/mapper.jl:318-462 restated).

match, best_kp and best_dist must be equal to the model, proj_yx within 1e-9 px with the same NaN pattern.  Exact equality is meaningful only
where no gate is decided by the last bits, so every parity test first asserts the model's margin >= 1e-9 on its scene (a condition on the
inputs, four orders of magnitude below what the generator gives; see np_local_map).  The shapes are the smallest at which the kernel can go
wrong: a 4 x 5 grid with partial last cells, M = 397 (no multiple of a group or a wave), a crowded patch that wraps the slot loop for every
group width, a grid that divides the image exactly (centre cells outside it), empty inputs, a ragged batch with an empty stream."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_local_map as npl  # noqa: E402

pytestmark = pytest.mark.gpu

DIST = (-0.28, 0.07, 2e-4, 2e-5)
SHAPES = {
    "plain": dict(seed=0),
    "plain_seed1": dict(seed=1),
    "distorted": dict(seed=0, distortion=DIST),
    "doubled": dict(seed=2, nb_3d=10),
    "crowd": dict(seed=0, crowd=80, M=300),
    "exact_grid": dict(seed=1, H=140, W=175),
    "small_a": dict(seed=3, N=40, M=61, K=3),
    "no_keypoints": dict(seed=4, N=0, M=61),
    "no_local_map": dict(seed=5, N=40, M=0),
}
_CACHE = {}


def scene(syn, name):
    """(scene, model result) of a named shape, computed once and shared (read-only)"""
    if name not in _CACHE:
        s = syn.local_map_scene(**SHAPES[name])
        if name == "exact_grid":
            _add_bottom_row(s)
        _CACHE[name] = (s, npl.do_local_map_matching(s["frame"], s["keypoints"], s["keyframes"], s["local_map"], s["params"]))
    return _CACHE[name]


def _world(frame, pixel, depth):
    cam, Twc = frame["cam"], np.linalg.inv(frame["Tcw"])
    xc = np.array([(pixel[1] - cam[2]) / cam[0] * depth, (pixel[0] - cam[3]) / cam[1] * depth, depth])
    return Twc[:3, :3] @ xc + Twc[:3, 3]


def _add_bottom_row(s):
    """H = 140 = 4 x 35: local-map points whose projection rounds to y = 140 have their centre cell in row 5, outside the grid; keypoints just
    above them (y = 139.1, row 4) are still within reach through the row above the centre"""
    rng = np.random.default_rng(7)
    for x in (20.3, 69.8, 101.2, 150.6):
        d = s["keypoints"][0]["descriptors"] if len(s["keypoints"][0]["descriptors"]) else s["keypoints"][1]["descriptors"]
        s["keypoints"].append({"pixel": (139.1, x), "descriptors": d.copy(), "observers": []})
        for dy in (0.55, 0.8):
            s["local_map"].append({"position": _world(s["frame"], (139.1 + dy, x + rng.uniform(-0.3, 0.3)), 6.0), "descriptors": d.copy(), "observers": []})


def check(out, ref):
    assert ref["margin"] >= 1e-9, ref["margin"]
    assert np.array_equal(out["match"], ref["match"])
    assert np.array_equal(out["best_kp"], ref["best_kp"])
    assert np.array_equal(out["best_dist"], ref["best_dist"])
    assert np.array_equal(np.isnan(out["proj_yx"]), np.isnan(ref["proj_yx"]))
    ok = ~np.isnan(ref["proj_yx"])
    assert np.all(np.abs(out["proj_yx"][ok] - ref["proj_yx"][ok]) <= 1e-9)


def call(slam, s):
    return slam.local_map_matching(s["frame"], s["keypoints"], s["keyframes"], s["local_map"], s["params"])


@pytest.mark.parametrize("name", ["plain", "plain_seed1", "distorted", "doubled", "crowd", "exact_grid"])
def test_matches_the_model(slam, syn, name):
    s, ref = scene(syn, name)
    c = ref["count"]
    print(name, "margin %.2e" % ref["margin"], "matched", int((ref["match"] >= 0).sum()), c)
    # the scene exercises what it is there for (properties of the inputs, read from the model)
    assert (ref["match"] >= 0).sum() >= 20 and c["contested"] > 0 and c["average"] > 0 and c["overlap"] > 0 and c["gated"] > 0
    assert c["ties_forward"] > 0 and c["ties_reverse"] > 0
    if name == "crowd":
        grid, rows, cols = npl.build_grid(s["frame"], s["keypoints"])
        crowded = [len(npl.get_surrounding_keypoints(grid, rows, cols, p, 35)) for p in ref["proj_yx"] if not np.isnan(p[0])]
        assert sum(n > 64 for n in crowded) >= 30, "the slot loop must wrap for a group of 64 lanes too"
    if name == "exact_grid":
        rows5 = [m for m, p in enumerate(ref["proj_yx"]) if not np.isnan(p[0]) and npl.to_cartesian(p, 35)[0] == 5]
        assert len(rows5) >= 4 and any(ref["best_kp"][m] >= 0 for m in rows5)
    if name == "doubled":
        far = [m for m in range(len(ref["best_kp"])) if ref["best_kp"][m] >= 0
               and np.hypot(*(ref["proj_yx"][m] - np.array(s["keypoints"][ref["best_kp"][m]]["pixel"]))) > 2.0]
        assert far, "a match beyond the undoubled distance"
    check(call(slam, s), ref)


def test_degenerate_inputs(slam, syn):
    for name in ("no_local_map", "no_keypoints"):
        s, ref = scene(syn, name)
        out = call(slam, s)
        assert out["match"].shape == (len(s["keypoints"]),) and out["best_kp"].shape == (len(s["local_map"]),)
        assert (out["match"] == -1).all() and (out["best_kp"] == -1).all() and np.isnan(out["proj_yx"]).all()
        assert np.array_equal(out["best_dist"], ref["best_dist"])
    s, _ = scene(syn, "small_a")
    # every target behind the camera
    Twc = np.linalg.inv(s["frame"]["Tcw"])
    behind = [dict(m, position=Twc[:3, :3] @ np.array([0.1 * i, -0.2, -3.0 - i]) + Twc[:3, 3]) for i, m in enumerate(s["local_map"])]
    ref = npl.do_local_map_matching(s["frame"], s["keypoints"], s["keyframes"], behind, s["params"])
    assert ref["count"]["gated"] == len(behind)
    out = slam.local_map_matching(s["frame"], s["keypoints"], s["keyframes"], behind, s["params"])
    check(out, ref)
    assert (out["match"] == -1).all() and np.isnan(out["proj_yx"]).all()
    # nobody has descriptors: projections are reported, nothing is taken
    bare = [dict(k, descriptors=np.zeros((0, 4), dtype=np.uint64)) for k in s["keypoints"]]
    ref = npl.do_local_map_matching(s["frame"], bare, s["keyframes"], s["local_map"], s["params"])
    out = slam.local_map_matching(s["frame"], bare, s["keyframes"], s["local_map"], s["params"])
    check(out, ref)
    assert (out["match"] == -1).all() and (out["best_kp"] == -1).all() and (~np.isnan(out["proj_yx"][:, 0])).sum() > 5


def test_batch_equals_single_calls(slam, syn):
    """streams of (M, N) = (397, 150), (0, 40), (61, 0) and a small live one behind the two empty ones: array for array the single calls"""
    names = ["plain", "no_local_map", "no_keypoints", "small_a"]
    scenes = [scene(syn, n)[0] for n in names]
    outs = slam.local_map_matching_batch([(s["frame"], s["keypoints"], s["keyframes"], s["local_map"], s["params"]) for s in scenes])
    assert len(outs) == 4
    for n, s, out in zip(names, scenes, outs):
        single = call(slam, s)
        for k in ("match", "best_kp", "best_dist", "proj_yx"):
            assert np.array_equal(out[k], single[k], equal_nan=True), (n, k)
        check(out, scene(syn, n)[1])
    assert (outs[3]["match"] >= 0).sum() > 3                     # the stream behind the empty ones reads its own slices


def test_two_calls_give_identical_outputs(slam, syn):
    s, _ = scene(syn, "crowd")
    a, b = call(slam, s), call(slam, s)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_rendered_frames_end_to_end(slam, syn, texture):
    """slam.describe of a frame and of its copy shifted by (2, -3) px feed kp_desc / mp_desc unchanged; map points on a fronto-parallel plane
    project 0.5 .. 4 px beside their keypoint: the ones inside the 2-px gate re-match, and the result is exactly the model's."""
    H, W, shift = 120, 160, np.array([2, -3])
    L, _, flows = texture(H, W, n=2, seed=0, step=(2.0, -3.0))
    assert flows[1] == (2.0, -3.0)
    e = slam.Extractor(200, 17, (-(-H // 35), -(-W // 35)), 35)
    kp0 = slam.detect(e, L[0], np.zeros((0, 2)))
    d0, k0 = slam.describe(e, L[0], kp0)
    d1, k1 = slam.describe(e, L[1], k0 + shift)
    row1 = {tuple(p): i for i, p in enumerate(k1)}
    both = [(i, row1[tuple(p + shift)]) for i, p in enumerate(k0) if tuple(p + shift) in row1]
    assert len(both) >= 40
    cam = np.array([100.0, 100.0, 80.0, 60.0, 0, 0, 0, 0, H, W])
    frame = {"Tcw": np.eye(4), "cam": cam, "cell_size": 35, "nb_3d_kpts": 100}
    keyframes = np.stack([np.eye(4), np.eye(4)])
    keyframes[0, :3, 3] = (0.4, 0.1, 0.0); keyframes[1, :3, 3] = (-0.3, 0.0, 0.1)
    rng = np.random.default_rng(3)
    keypoints, local_map, inside, proj = [], [], [], []
    view_thr = np.cos(np.arctan(max(0.5 * H / cam[1], 0.5 * W / cam[0])))
    for n, (i0, i1) in enumerate(both):
        px = k1[i1].astype(float)
        Xw = _world(frame, px, 5.0)
        c = keyframes[0][:3, :3] @ Xw + keyframes[0][:3, 3]
        keypoints.append({"pixel": tuple(px), "descriptors": d1[i1:i1 + 1], "observers": [(0, (100.0 * c[1] / c[2] + 60.0, 100.0 * c[0] / c[2] + 80.0))]})
        r = (0.5, 1.0, 1.5, 3.0, 4.0)[n % 5]
        a = rng.uniform(0, 2 * np.pi)
        q = px + r * np.array([np.sin(a), np.cos(a)])
        local_map.append({"position": _world(frame, q, 5.0), "descriptors": d0[i0:i0 + 1], "observers": [1]})
        proj.append(q)
        # inside the gates of mapper.jl:345-352, :407-408, :445 -- worked out here from the geometry and the two descriptors, not read from a result:
        # the pixel offset under max_projection_distance, the point in the image and not beyond the view-angle threshold (the corners of this
        # camera are: 0.5 W / fx = 0.8 -> 38.7 degrees), the descriptor pair within 0.35 * 256 bits
        ny, nx = (q[0] - cam[3]) / cam[1], (q[1] - cam[2]) / cam[0]
        bits = sum(bin(int(u) ^ int(v)).count("1") for u, v in zip(d0[i0], d1[i1]))
        inside.append(r < 2.0 and 1.0 / np.sqrt(1.0 + nx * nx + ny * ny) > view_thr + 1e-6 and 1.01 <= q[0] <= H - 0.01 and 1.01 <= q[1] <= W - 0.01
                      and bits <= 256 * 0.35)
    inside, proj = np.array(inside), np.array(proj)
    # a pair is alone when no other keypoint is within the gate of its point's projection and its keypoint within the gate of no other point's
    D = np.hypot(proj[:, None, 0] - k1[[b[1] for b in both]][None, :, 0], proj[:, None, 1] - k1[[b[1] for b in both]][None, :, 1]) <= 2.0 + 1e-6
    alone = np.array([D[n].sum() <= 1 and D[:, n].sum() <= 1 for n in range(len(both))])
    params = slam.Params()
    ref = npl.do_local_map_matching(frame, keypoints, keyframes, local_map, params)
    out = slam.local_map_matching(frame, keypoints, keyframes, local_map, params)
    print("pairs", len(both), "inside", int(inside.sum()), "alone", int(alone.sum()), "matched", int((out["match"] >= 0).sum()),
          "inside but unmatched", np.flatnonzero(inside & (out["match"] < 0)))
    check(out, ref)
    assert (inside & alone).sum() >= 20
    own = np.arange(len(both))
    assert (out["match"][inside & alone] >= 0).all(), "a keypoint whose map point projects inside the gates is re-attached"
    assert (out["match"][inside & alone] == own[inside & alone]).all() and (out["best_kp"][inside & alone] == own[inside & alone]).all()
    far = np.array([(0.5, 1.0, 1.5, 3.0, 4.0)[n % 5] > 2.0 for n in own])
    assert (out["best_kp"][far] != own[far]).all()                              # a point outside the gate never takes its own keypoint


def test_argument_errors_launch_nothing(slam, syn):
    s, _ = scene(syn, "small_a")
    ctx = slam.default_context(0)
    p = slam.pack_local_map(s["frame"], s["keypoints"], s["keyframes"], s["local_map"], s["params"])
    ctx.prof_enable(True); ctx.prof_reset()
    try:
        bad = dict(p, mp_desc_off=p["mp_desc_off"].copy())
        bad["mp_desc_off"][5] = bad["mp_desc_off"][4] - 1
        with pytest.raises(slam.SlamHipError, match="mp_desc_off decreases"):
            slam.local_map_matching_packed(bad, ctx)
        bad = dict(p, kp_obs_kf=p["kp_obs_kf"].copy())
        bad["kp_obs_kf"][0] = p["K"]
        with pytest.raises(slam.SlamHipError, match="no row of its 3 key-frames"):
            slam.local_map_matching_packed(bad, ctx)
        bad = dict(p, mp_obs_kf=p["mp_obs_kf"].copy())
        bad["mp_obs_kf"][-1] = -1
        with pytest.raises(slam.SlamHipError, match="mp_obs_kf"):
            slam.local_map_matching_packed(bad, ctx)
        c, kp_off, kf_off, mp_off = slam.concat_packs([p, p])
        a, _ = slam.local_map._args(c)
        kp_off[1] = kp_off[2] + 1
        import ctypes as C
        rc = ctx.lib.slam_local_map_match_batch(ctx.h, 2, kp_off.ctypes.data_as(slam._lib.i32p), kf_off.ctypes.data_as(slam._lib.i32p),
                                                mp_off.ctypes.data_as(slam._lib.i32p), C.byref(a))
        assert rc != 0 and b"kp_offsets decreases" in ctx.lib.slam_last_error(ctx.h)
        assert ctx.prof_get("local_map_match")[1] == 0, "no span was opened: nothing was copied or launched"
        slam.local_map_matching_packed(p, ctx)
        assert ctx.prof_get("local_map_match")[1] == 1
    finally:
        ctx.prof_enable(False)
