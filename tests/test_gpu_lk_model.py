"""GPU: the tracking kernels point for point against the long-double model of tests/hp_lk.py.

Two PyramidBatch objects (S = 4, levels = 3) per shape are built in TOLERANCE mode from u8 frames; all six planes of every level of
every member are downloaded and handed to the model and -- copied into oracle.Pyramid objects -- to the C oracle, so plane error plays
no part: the three implementations track on the same numbers.  Per case (shape x window x prior mode, hp_lk: the cases):

  fate       equal on every point that is not excused (decision margin > 1e-6); at most 1 % of the case's points are excused
  positions  E_hip = max |x - model| <= 64 * max(E_seq, E_wave, ulp(max(H, W))), E_seq / E_wave the C oracle's two summation orders on
             the same planes and points; never above 1e-6 px (`<.., true>`) / 1e-9 px (exact kernels)

through hp_lk.check, the assertion test_lk_model_host.py proves sensitive (a position moved by 1e-9 px, one pixel raised by 2^-20,
swapped gradients, window +- 1, a cleared status: all rejected).  Kernels reached: k_kpset_match<3 | 6 | 9, true> (windows 5 / 9 / 11,
and 12 on the 9-slot kernel's uncached path) in temporal and stereo mode, and on the same planes the exact k_fb_track (per-point
displacement) and k_flow_match; k_kpset_match<.., false> through two batches built in exact mode.  Every case prints one line
(`ROW ...`, run with -s): the table of DESIGN 3.3.1 is made of them."""
import numpy as np
import pytest

import hp_lk as hp

pytestmark = pytest.mark.gpu
_WORLD = {}
ROW = {5: "<3, true>", 9: "<6, true>", 11: "<9, true> cached", 12: "<9, true> window 12"}


def _batch(slam, frames_u8, H, W, fast):
    import torch
    dev = torch.from_numpy(np.stack([np.ascontiguousarray(f.T) for f in frames_u8])).cuda()
    torch.cuda.synchronize()
    pb = slam.PyramidBatch((H, W), levels=3, S=hp.S)
    pb.update_([dev.data_ptr() + s * H * W for s in range(hp.S)], u8=True, fast=fast)
    return pb, dev


def world(slam, orc, syn, shape):
    """batches (tolerance + exact mode) of frame 0 / frame 1 / right frame 1, their downloaded planes, the oracle's copies, the points"""
    if shape not in _WORLD:
        H, W = hp.SHAPES[shape]
        frs = hp.frames(syn, shape)
        w = dict(frs=frs, pts=hp.points(orc, shape, frs), models={}, keep=[])
        for kind, fast in (("tol", True), ("exact", False)):
            for key in ("a", "b", "r"):
                if key == "r" and not (shape == "even" and fast):
                    continue
                pb, dev = _batch(slam, [f[key] for f in frs], H, W, fast)
                w["keep"].append(dev)
                w[kind, key] = pb
                w[kind, key, "planes"] = [hp.planes_of(pb.pyramids[s]) for s in range(hp.S)]
                w[kind, key, "orc"] = [p.to_oracle(orc) for p in w[kind, key, "planes"]]
        _WORLD[shape] = w
    return _WORLD[shape]


def model_of(w, kind, s, window, to="b", frm="a"):
    k = (kind, frm, to, s, window)
    if k not in w["models"]:
        w["models"][k] = hp.Model(w[kind, frm, "planes"][s], w[kind, to, "planes"][s], window, 1.0)
    return w["models"][k]


def kept_form(r):
    """the keypoint set only shows kept / lost: fate 1 (updated) and 2 (kept as it is) fold into 1; positions stay"""
    return dict(r, fate=(r["fate"] > 0).astype(np.int64))


def kpset_flow(slam, w, kind, shape, window, levels3d, pr, stereo=False):
    """upload the case's four lists (ids = arange), one slam_kpset_flow_match / _stereo_match, the lists back in the model's terms"""
    ks = slam.KeypointSet(hp.S, max(len(p) for p in w["pts"]) + 8)
    for s in range(hp.S):
        ks.upload(s, w["pts"][s], pr[s][0], xyz=hp.xyz_of(pr[s][1]), ids=np.arange(len(w["pts"][s])))
    params = slam.Params(window_size=window, pyramid_levels=3, max_ktl_distance=1.0)
    sp = slam.stream_params(hp.S, Tcw=np.eye(4), cam=hp.IDENTITY_CAM)
    if stereo:
        ks.stereo_match(w[kind, "b"], w[kind, "r"], params, sp, prior=1, pyramid_levels_3d=levels3d, epipolar_error=2.0)
    else:
        ks.flow_match(w[kind, "a"], w[kind, "b"], params, sp, prior=1, pyramid_levels_3d=levels3d)
    out, raw = [], []
    for s in range(hp.S):
        d = ks.download(s)
        n = len(w["pts"][s])
        fate = np.zeros(n, np.int64); pos = np.full((n, 2), np.nan)
        assert len(np.unique(d["ids"])) == len(d["ids"]) and np.array_equal(d["ids"], np.sort(d["ids"]))       # stable compaction
        if stereo:
            assert np.array_equal(d["yx"], w["pts"][s][d["ids"]])                                               # positions untouched
            fate[d["ids"]] = np.where(d["has_stereo"], 1, 2)
            pos[d["ids"]] = np.where(d["has_stereo"][:, None], d["stereo_yx"], d["yx"])
        else:
            fate[d["ids"]] = 1; pos[d["ids"]] = d["yx"]
        out.append(hp.result(fate, pos)); raw.append(d)
    ks.close()
    return hp.concat(out), raw


def yardsticks(orc, w, kind, mod, pr, shape, window, levels3d, stereo=False, fold=True):
    frm, to = ("b", "r") if stereo else ("a", "b")
    E = []
    for order in (0, 1):
        got = hp.concat([hp.oracle_matching(orc, w[kind, frm, "orc"][s], w[kind, to, "orc"][s], w["pts"][s], pr[s][0], pr[s][1], hp.SHAPES[shape],
                                            window, 3, levels3d, order, stereo=stereo) for s in range(hp.S)])
        E.append(hp.check(mod, kept_form(got) if fold else got, 0.0, 0.0, hp.SHAPES[shape], hp.E_ORACLE_MAX, ("oracle", order))[0])
    return E


def report(row, shape, window, mode, E_seq, E_wave, E_hip, nex, n):
    yard = max(E_seq, E_wave, hp.ulp(max(hp.SHAPES[shape])))
    print(f"\nROW {row} | {shape} w{window} {mode} | n={n} excused={nex} E_seq={E_seq:.2e} E_wave={E_wave:.2e} E_hip={E_hip:.2e} r={E_hip / yard:.2f}")


@pytest.mark.parametrize("mode", hp.MODES)
@pytest.mark.parametrize("window", hp.WINDOWS)
@pytest.mark.parametrize("shape", list(hp.SHAPES))
def test_tolerance_kpset_match_vs_model(slam, orc, syn, shape, window, mode):
    """slam_kpset_flow_match between two tolerance-mode batches: k_kpset_match<3 | 6 | 9, true>, four streams, every prior mode"""
    w = world(slam, orc, syn, shape)
    HW = hp.SHAPES[shape]
    levels3d = hp.mode_levels(mode)[0]
    pr = hp.priors(shape, w["frs"], w["pts"], window, mode)
    full = hp.concat([model_of(w, "tol", s, window).matching(w["pts"][s], pr[s][0], pr[s][1], HW, 3, levels3d) for s in range(hp.S)])
    mod = kept_form(full)
    E_seq, E_wave = yardsticks(orc, w, "tol", mod, pr, shape, window, levels3d)
    got, raw = kpset_flow(slam, w, "tol", shape, window, levels3d, pr)
    E_hip, nex = hp.check(mod, got, E_seq, E_wave, HW, hp.CAP_TOL, (shape, window, mode))
    report("k_kpset_match" + ROW[window], shape, window, mode, E_seq, E_wave, E_hip, nex, len(mod["fate"]))
    # a 3-D keypoint whose prior projects outside the image is neither tracked nor removed (map_manager.jl:501-506)
    gate = full["fate"] == 2
    assert gate.sum() >= 1 and (got["fate"][gate] == 1).all()
    assert np.array_equal(got["pos"][gate], np.concatenate(w["pts"])[gate])
    assert (full["fate"] == 0).sum() >= 1 and (full["fate"] == 1).sum() >= 30


@pytest.mark.parametrize("mode", hp.MODES)
@pytest.mark.parametrize("window", hp.WINDOWS)
@pytest.mark.parametrize("shape", list(hp.SHAPES))
def test_exact_kernels_on_tolerance_planes_vs_model(slam, orc, syn, shape, window, mode):
    """members 0 and 3 of the tolerance-mode batches through the exact kernels: fb_tracking_ with a per-point displacement
    (k_fb_track) and the array protocol (k_flow_match)"""
    w = world(slam, orc, syn, shape)
    HW = hp.SHAPES[shape]
    levels3d = hp.mode_levels(mode)[0]
    pr = hp.priors(shape, w["frs"], w["pts"], window, mode)
    members = (0, 3)
    A, B = w["tol", "a"].pyramids, w["tol", "b"].pyramids
    OA, OB = w["tol", "a", "orc"], w["tol", "b", "orc"]
    # ---- k_fb_track ----
    disp = {s: (1.0 / 2.0 ** levels3d) * (pr[s][1] - w["pts"][s]) for s in members}
    mod = hp.concat([model_of(w, "tol", s, window).fb_tracking(w["pts"][s], disp[s], levels3d) for s in members])
    E = [hp.check(mod, hp.concat([hp.oracle_fb(orc, OA[s], OB[s], w["pts"][s], disp[s], window, levels3d, order) for s in members]),
                  0.0, 0.0, HW, hp.E_ORACLE_MAX, ("oracle fb", order))[0] for order in (0, 1)]
    got = []
    for s in members:
        out, st = slam.fb_tracking_(A[s], B[s], w["pts"][s], displacement=disp[s], pyramid_levels=levels3d, window_size=window, max_distance=1.0)
        got.append(hp.result(st, out))
    E_hip, nex = hp.check(mod, hp.concat(got), E[0], E[1], HW, hp.CAP_EXACT, (shape, window, mode, "k_fb_track"))
    report("k_fb_track", shape, window, mode, E[0], E[1], E_hip, nex, len(mod["fate"]))
    # ---- k_flow_match ----
    params = slam.Params(window_size=window, pyramid_levels=3, max_ktl_distance=1.0)
    mod = hp.concat([model_of(w, "tol", s, window).matching(w["pts"][s], pr[s][0], pr[s][1], HW, 3, levels3d) for s in members])
    E = [hp.check(mod, hp.concat([hp.oracle_matching(orc, OA[s], OB[s], w["pts"][s], pr[s][0], pr[s][1], HW, window, 3, levels3d, order) for s in members]),
                  0.0, 0.0, HW, hp.E_ORACLE_MAX, ("oracle match", order))[0] for order in (0, 1)]
    got = []
    for s in members:
        px, (is3, proj) = w["pts"][s], pr[s]
        if levels3d == 1:                                    # the frame-level seam (its 3-D attempt is fixed at one level, as the reference's)
            r = slam.optical_flow_matching_frame(A[s], B[s], px, is3, proj, params, HW)
            fate = np.where(r["updated"], 1, np.where(r["removed"], 0, 2)); pos = r["new_pixels"]
        else:
            inside = (proj[:, 0] >= 1) & (proj[:, 0] <= HW[0]) & (proj[:, 1] >= 1) & (proj[:, 1] <= HW[1])
            sel = np.flatnonzero(~(is3 & ~inside))
            new, st = slam.optical_flow_matching(A[s], B[s], px[sel], is3[sel], proj[sel], params, pyramid_levels_3d=levels3d)
            fate = np.full(len(px), 2); pos = px.copy()
            fate[sel] = st; pos[sel] = new
        got.append(hp.result(fate, pos))
    E_hip, nex = hp.check(mod, hp.concat(got), E[0], E[1], HW, hp.CAP_EXACT, (shape, window, mode, "k_flow_match"))
    report("k_flow_match", shape, window, mode, E[0], E[1], E_hip, nex, len(mod["fate"]))


@pytest.mark.parametrize("mode", hp.MODES)
@pytest.mark.parametrize("window", hp.WINDOWS)
@pytest.mark.parametrize("shape", list(hp.SHAPES))
def test_exact_kpset_match_vs_model(slam, orc, syn, shape, window, mode):
    """k_kpset_match<.., false>: the same lists between two batches built in exact mode (their own planes, their own model runs)"""
    w = world(slam, orc, syn, shape)
    HW = hp.SHAPES[shape]
    levels3d = hp.mode_levels(mode)[0]
    pr = hp.priors(shape, w["frs"], w["pts"], window, mode)
    mod = kept_form(hp.concat([model_of(w, "exact", s, window).matching(w["pts"][s], pr[s][0], pr[s][1], HW, 3, levels3d) for s in range(hp.S)]))
    E_seq, E_wave = yardsticks(orc, w, "exact", mod, pr, shape, window, levels3d)
    got, raw = kpset_flow(slam, w, "exact", shape, window, levels3d, pr)
    E_hip, nex = hp.check(mod, got, E_seq, E_wave, HW, hp.CAP_EXACT, (shape, window, mode))
    report("k_kpset_match exact", shape, window, mode, E_seq, E_wave, E_hip, nex, len(mod["fate"]))


def test_tolerance_kpset_stereo_match_vs_model(slam, orc, syn):
    """slam_kpset_stereo_match, even, window 9, disparity 6.3, epipolar_error 2.0, identity undistortion: matched / unmatched /
    observation removed per point, (left row, matched column) within the bound"""
    shape, window = "even", 9
    w = world(slam, orc, syn, shape)
    HW = hp.SHAPES[shape]
    pr = hp.priors(shape, w["frs"], w["pts"], window, "l1", seed=1, shift=(0.0, -hp.DISPARITY))
    mod = hp.concat([model_of(w, "tol", s, window, to="r", frm="b").matching(w["pts"][s], pr[s][0], pr[s][1], HW, 3, 1, stereo=True,
                                                                              undistorted_left=w["pts"][s]) for s in range(hp.S)])
    E_seq, E_wave = yardsticks(orc, w, "tol", mod, pr, shape, window, 1, stereo=True, fold=False)
    got, raw = kpset_flow(slam, w, "tol", shape, window, 1, pr, stereo=True)
    E_hip, nex = hp.check(mod, got, E_seq, E_wave, HW, hp.CAP_TOL, "stereo")
    report("stereo", shape, window, "l1", E_seq, E_wave, E_hip, nex, len(mod["fate"]))
    assert (mod["fate"] == 0).sum() >= 1 and (mod["fate"] == 2).sum() >= 1 and (mod["fate"] == 1).mean() > 0.3
    up = got["fate"] == 1
    assert np.array_equal(got["pos"][up][:, 0], np.concatenate(w["pts"])[up][:, 0])                    # the left keypoint's row is kept


@pytest.mark.parametrize("window", hp.WINDOWS)
def test_same_call_twice_gives_byte_equal_lists(slam, orc, syn, window):
    w = world(slam, orc, syn, "odd")
    pr = hp.priors("odd", w["frs"], w["pts"], window, "l0")
    runs = [kpset_flow(slam, w, "tol", "odd", window, 0, pr)[1] for _ in range(2)]
    for s in range(hp.S):
        for k in ("yx", "ids", "is_3d"):
            assert runs[0][s][k].tobytes() == runs[1][s][k].tobytes(), (s, k)
    we = world(slam, orc, syn, "even")
    pr = hp.priors("even", we["frs"], we["pts"], window, "l1", seed=1, shift=(0.0, -hp.DISPARITY))
    runs = [kpset_flow(slam, we, "tol", "even", window, 1, pr, stereo=True)[1] for _ in range(2)]
    for s in range(hp.S):
        m = runs[0][s]["has_stereo"]
        assert m.tobytes() == runs[1][s]["has_stereo"].tobytes() and runs[0][s]["ids"].tobytes() == runs[1][s]["ids"].tobytes()
        assert runs[0][s]["stereo_yx"][m].tobytes() == runs[1][s]["stereo_yx"][m].tobytes()
