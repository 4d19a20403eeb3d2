"""GPU: slam_kpset_frame_stats -- the per-stream counts, occupied cells, mean and exact median parallax that check_new_kf_required /
check_ready_for_init! read (front_end.jl:343-452, frame.jl:321-337) -- against the numpy model of tests/np_kf.py, on lists that go in through
KeypointSet.upload / upload_keyframe (no images, no pyramids).

Exact scenes: camera (1, 1, 0, 0) without distortion and integer key-frame pixels with offsets (3k, 4k), (5k, 12k) or (t, 0), so every parallax is
exactly representable and the sums are exact in any order: everything is compared with array_equal.  General scenes: a KITTI camera with lens
distortion and a 2 degree compensation: counts and cells equal, mean / median within 1e-9 px (the project's bar for projected pixels; the median
is 1-Lipschitz in the terms, so the per-term bar carries over).

upload() clears the stereo flags and the set has no upload for them, so nb_stereo_kpts is 0 here; tests/test_gpu_adaptive_keyframes.py compares
it on lists that went through the stereo match."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_kf  # noqa: E402

pytestmark = pytest.mark.gpu

CAM1, NODIST = (1.0, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0)
CAP = 5000                                                       # not a multiple of 64; above the kernel's 4096-term LDS array
SIZES = (0, 1, 2, 3, 255, 256, 257, 4096, 4097)                  # n_parallax: chunk edges of the 256-thread loops, the LDS / HBM threshold
PATTERNS = ("random", "all_equal", "middle_equal", "middle_adjacent", "dup300")
H0, W0, CELL0 = 370, 1226, 35


def _offsets(rng, m, pattern):
    """(m, 2) offsets yx - kyx whose norms are exactly representable, and whether the SUM of the norms is exact in any order"""
    k = rng.integers(0, 60, m)
    kind = rng.integers(0, 3, m)
    t = np.where(kind == 0, 5 * k, np.where(kind == 1, 13 * k, k)).astype(np.float64)
    if pattern == "all_equal":                                   # a stationary camera: every parallax 0
        return np.zeros((m, 2)), True
    if pattern == "middle_equal" and m >= 4:                     # the two middle order statistics are the same value
        lo = (m - 1) // 2
        t = np.concatenate([rng.integers(0, 100, lo), [100.0, 100.0], rng.integers(101, 200, m - lo - 2)]).astype(np.float64)
        kind = np.full(m, 2)
    exact = True
    if pattern == "middle_adjacent" and m >= 4:                  # ... adjacent doubles: the median is lo / 2 + hi / 2 of them
        lo = (m - 1) // 2
        a = 100.5
        t = np.concatenate([rng.integers(0, 100, lo), [a, np.nextafter(a, np.inf)], rng.integers(101, 200, m - lo - 2)]).astype(np.float64)
        kind = np.full(m, 2); exact = False
    if pattern == "dup300" and m >= 400:                         # 300 copies of the median value 256.0, whose neighbours below (255, 254 ...) differ
        lo = (m - 300) // 2                                      # from it in the second radix byte (0x406F.. / 0x4070..)
        t = np.concatenate([rng.integers(250, 256, lo), np.full(300, 256.0), rng.integers(257, 262, m - 300 - lo)]).astype(np.float64)
        kind = np.full(m, 2)
    p = rng.permutation(m)
    t, kind = t[p], kind[p]
    d = np.zeros((m, 2))
    for q, (a, b) in enumerate(((3, 4), (5, 12))):
        sel = kind == q
        d[sel, 0] = a * (t[sel] / (5, 13)[q]); d[sel, 1] = b * (t[sel] / (5, 13)[q])
    d[kind == 2, 0] = t[kind == 2]
    d *= rng.choice([-1.0, 1.0], size=(m, 2))
    return d, exact


def _stream(rng, m, pattern, extra=0, special=None):
    """a list with m keypoints the key-frame observes (a mixed is3d pattern) and `extra` it does not, shuffled"""
    n = m + extra
    d, exact = _offsets(rng, m, pattern)
    kyx = np.zeros((n, 2)); yx = np.zeros((n, 2))
    kyx[:m] = np.stack([rng.integers(0, H0, m), rng.integers(0, W0, m)], axis=1)
    kyx[:m][(d != np.round(d)).any(axis=1)] = 0.0              # a non-integer offset stays exact only against a zero key-frame pixel
    yx[:m] = kyx[:m] + d
    yx[m:] = np.stack([rng.integers(0, H0, extra), rng.integers(0, W0, extra)], axis=1) + 0.25
    kyx[m:] = -7.0                                               # never read: haskf = 0
    haskf = np.arange(n) < m
    is3d = rng.random(n) < 0.4
    if special == "nan" and m:
        kyx[m // 2, 1] = np.nan
    p = rng.permutation(n)
    return dict(yx=yx[p], kyx=kyx[p], haskf=haskf[p], is3d=is3d[p], exact=exact)


EMPTY = dict(yx=np.zeros((0, 2)), kyx=np.zeros((0, 2)), haskf=np.zeros(0, bool), is3d=np.zeros(0, bool), exact=True)


def _fill(ks, streams):
    for s, L in enumerate(streams):
        ks.upload(s, L["yx"], L["is3d"])
        ks.upload_keyframe(s, L["kyx"], L["haskf"])


def _model(streams, cam, dist, flags, cell, H, W, R=None):
    return np.stack([np_kf.frame_stats(cam, dist, L["yx"], L["is3d"], np.zeros(len(L["yx"]), bool), L["kyx"], L["haskf"], flags, cell, H, W, R) for L in streams])


def _check_exact(got, want, streams, tag):
    for s, L in enumerate(streams):
        cols = list(range(8)) if L["exact"] else [0, 1, 2, 3, 4, 5, 7]
        assert np.array_equal(got[s, cols], want[s, cols], equal_nan=True), (tag, s, got[s], want[s])
        if not L["exact"]:                                       # the sum of these terms is not exact: its order is the implementation's
            assert abs(got[s, 6] - want[s, 6]) <= 1e-9, (tag, s, got[s, 6], want[s, 6])


@pytest.fixture(scope="module")
def ks5(slam):
    ks = slam.KeypointSet(5, CAP)
    yield ks
    ks.close()


@pytest.mark.parametrize("round_", [0, 1, 2])
def test_exact_scenes_five_streams(slam, ks5, round_):
    """stream 0 empty; over three fillings of one set: every n_parallax of SIZES (chunk edges, the LDS / HBM threshold) and every value pattern"""
    rng = np.random.default_rng(100 + round_)
    sizes = ((0, 1, 2, 3), SIZES[5:9], (4096, 4097, 1000, 255))[round_]
    pats = (("random",) * 4, ("middle_equal", "middle_adjacent", "all_equal", "dup300"), ("middle_adjacent", "middle_equal", "dup300", "middle_adjacent"))[round_]
    # (round 0, stream 1: n > 0 but no key-frame observation at all: n_parallax 0, mean = median = 0)
    streams = [EMPTY] + [_stream(rng, m, p, extra=300 if (round_, i) == (0, 0) else (0, 37)[(i + round_) % 2]) for i, (m, p) in enumerate(zip(sizes, pats))]
    _fill(ks5, streams)
    sp = slam.stream_params(5, cam=CAM1, dist=NODIST)
    for flags in (0, 2):
        got = ks5.frame_stats(sp, flags, CELL0, (H0, W0))
        want = _model(streams, CAM1, NODIST, flags, CELL0, H0, W0)
        _check_exact(got, want, streams, (round_, flags))
    assert got[0].tolist() == [0.0] * 8
    if round_ == 0:
        assert got[1, 0] == 300 and got[1, 3] == 0 and got[1, 5:].tolist() == [0.0, 0.0, 0.0]


def test_exact_scenes_seventy_streams(slam):
    """more than one wave of streams: every stream is its own workgroup (stream 69 non-empty), sizes and patterns cycle over the streams"""
    S = 70
    rng = np.random.default_rng(7)
    streams = [EMPTY]
    for s in range(1, S):
        m = SIZES[s % len(SIZES)] if s != 69 else 4097
        streams.append(_stream(rng, m, PATTERNS[s % len(PATTERNS)], extra=(0, 11, 64)[s % 3]))
    ks = slam.KeypointSet(S, CAP)
    _fill(ks, streams)
    sp = slam.stream_params(S, cam=CAM1, dist=NODIST)
    for flags in (0, 2):
        got = ks.frame_stats(sp, flags, CELL0, (H0, W0))
        _check_exact(got, _model(streams, CAM1, NODIST, flags, CELL0, H0, W0), streams, flags)
    assert got[69, 5] > 0 and np.array_equal(ks.counts(), got[:, 0].astype(np.int32))
    ks.close()


def test_inf_and_nan_terms(slam, ks5):
    """one NaN term (a NaN in kyx): mean and median NaN.  One +inf term: the median is unaffected, the mean is +inf.  The lens model turns an
    infinite PIXEL into NaN (0 * inf in the distortion polynomial), so the infinite term comes from the compensated projection: with the
    'rotation' [1 0 0; 0 1 0; -1 0 1] the point at x = 1 projects through z = 0, and the points at x = 0 through z = 1, exactly."""
    rng = np.random.default_rng(3)
    nan_streams = [EMPTY, _stream(rng, 257, "random", special="nan"), _stream(rng, 4097, "random", extra=5, special="nan"), _stream(rng, 2, "random", special="nan"), EMPTY]
    _fill(ks5, nan_streams)
    sp = slam.stream_params(5, cam=CAM1, dist=NODIST)
    got = ks5.frame_stats(sp, 0, CELL0, (H0, W0)); want = _model(nan_streams, CAM1, NODIST, 0, CELL0, H0, W0)
    assert np.array_equal(got[:, :6], want[:, :6])
    assert np.isnan(got[1:4, 6:]).all() and np.isnan(want[1:4, 6:]).all() and got[0, 6:].tolist() == [0.0, 0.0]
    R = np.array([[1.0, 0, 0], [0, 1, 0], [-1, 0, 1]])
    streams = [EMPTY]
    for m in (256, 4097, 3, 300):
        k = rng.integers(0, 50, m).astype(np.float64)
        kyx = np.stack([rng.integers(0, H0, m), np.zeros(m)], axis=1).astype(np.float64)
        yx = np.stack([kyx[:, 0] + 3 * k, np.zeros(m)], axis=1); kyx[:, 1] = 4 * k         # through z = 1: (y, 0) - (ky, 4k) = (3k, -4k)
        j = m // 3
        yx[j] = (2.0, 1.0)                                                                  # through z = 0: (inf, inf)
        streams.append(dict(yx=yx, kyx=kyx, haskf=np.ones(m, bool), is3d=rng.random(m) < 0.3, exact=True))
    _fill(ks5, streams)
    T = np.tile(np.eye(4), (5, 1, 1)); T[:, :3, :3] = R
    sp = slam.stream_params(5, Tcw=T, cam=CAM1, dist=NODIST)
    got = ks5.frame_stats(sp, 1, CELL0, (H0, W0)); want = _model(streams, CAM1, NODIST, 1, CELL0, H0, W0, R)
    assert np.array_equal(got, want), (got, want)
    assert np.isposinf(got[1:, 6]).all() and np.isfinite(got[1:, 7]).all()


CELL_CASES = [(35, 370, 1226), (35, 1080, 1920), (7, 70, 70)]


@pytest.mark.parametrize("cell,H,W", CELL_CASES)
def test_occupied_cells(slam, ks5, cell, H, W):
    gr, gc = -(-H // cell), -(-W // cell)
    rng = np.random.default_rng(cell + H)
    cy, cx = np.meshgrid(np.arange(gr), np.arange(gc), indexing="ij")
    every = np.stack([cy.ravel() * cell + rng.uniform(-0.49, cell - 0.51, gr * gc), cx.ravel() * cell + rng.uniform(-0.49, cell - 0.51, gr * gc)], axis=1)
    c = float(cell)
    special = np.array([[c - 0.5, 1.0], [c + 0.5, 1.0], [c + 1.5, 1.0],                     # .5 goes to the even neighbour: for cell 35 -> 34, 36, 36
                        [c, 2 * c - 1.0], [2 * c - 1.0, c], [2 * c - 0.5, 2 * c - 0.5],         # both ends of a cell, and half a pixel past its end
                        [float(H), 3.0], [3.0, float(W)], [float(gr * cell), 3.0], [3.0, float(gc * cell)], [gr * cell - 0.51, gc * cell - 0.51],
                        [-0.4, -0.5], [-3.0, 5.0], [-c, 5.0], [5.0, -c - 1.0], [1e30, 5.0], [5.0, -1e30]])
    crowd = np.stack([rng.uniform(2 * c, 3 * c - 1, 700), rng.uniform(c, 2 * c - 1, 700)], axis=1)           # many keypoints, one cell
    lists = [every[rng.permutation(len(every))], special, crowd, np.concatenate([every, crowd, special]), np.zeros((0, 2))]
    streams = [dict(yx=yx, kyx=yx.copy(), haskf=np.zeros(len(yx), bool), is3d=np.zeros(len(yx), bool), exact=True) for yx in lists]
    _fill(ks5, streams)
    got = ks5.frame_stats(slam.stream_params(5, cam=CAM1, dist=NODIST), 1, cell, (H, W))
    want = _model(streams, CAM1, NODIST, 1, cell, H, W, np.eye(3))
    assert np.array_equal(got, want), (got[:, 4], want[:, 4])
    assert got[0, 4] == gr * gc and got[2, 4] == 1 and got[3, 4] == gr * gc and got[4, 4] == 0
    if (cell, H, W) == (35, 1080, 1920):
        assert gr * gc == 1705                                                              # more cells than a 1024-bit map would hold
    if (cell, H, W) == (7, 70, 70):
        only = dict(yx=np.array([[70.0, 3.0]]), kyx=np.zeros((1, 2)), haskf=np.zeros(1, bool), is3d=np.zeros(1, bool))
        ks5.upload(0, only["yx"], only["is3d"])
        assert ks5.frame_stats(slam.stream_params(5, cam=CAM1, dist=NODIST), 0, cell, (H, W))[0, 4] == 0      # y = 70 at H = 70: off the grid


# ---- general scenes ---------------------------------------------------------------------------------------------------------------------
DIST = (-0.08, 0.02, 8e-4, -5e-4)
MAXKP = 1000
# per stream: (keypoints, flow in px, share of 3-D keypoints, frames_delta, prev_kf_nb_3d, has_prev_kf)
GENERAL = [(700, (0.4, 2.5), 0.30, 3, 400, 1), (1100, (9.0, -22.0), 0.60, 1, 520, 1), (900, (-5.0, 12.0), 0.60, 6, 900, 1), (1000, (3.0, 4.0), 0.01, 2, 30, 1)]


def _rot(deg, axis):
    a = np.asarray(axis, dtype=np.float64); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


@pytest.fixture(scope="module")
def general(syn):
    rng = np.random.default_rng(11)
    streams = []
    for n, flow, f3, _, _, _ in GENERAL:
        kyx = np.stack([rng.uniform(5, H0 - 5, n), rng.uniform(5, W0 - 5, n)], axis=1)
        yx = kyx + np.asarray(flow) + rng.normal(0, 0.7, (n, 2))
        haskf = rng.random(n) < 0.85
        streams.append(dict(yx=yx, kyx=kyx, haskf=haskf, is3d=rng.random(n) < f3, exact=False))
    R = _rot(2.0, (0.3, 1.0, -0.2))
    cam = syn.KITTI_CAM
    want = {f: _model(streams, cam, DIST, f, CELL0, H0, W0, R) for f in (1, 3)}
    dec = [np_kf.decide(want[1][s], g[3], g[4], bool(g[5]), MAXKP, 20.0, False) for s, g in enumerate(GENERAL)]
    return dict(streams=streams, R=R, cam=cam, want=want, dec=dec)


def test_general_scene_model_is_away_from_its_thresholds(general):
    """CPU part, before any device result is looked at: every double comparison of the model's decisions is >= 1e-6 from its threshold, and the
    scenes reach more than one exit of the rule"""
    assert min(d[2] for d in general["dec"]) >= 1e-6, [d[2] for d in general["dec"]]
    assert len({d[1] for d in general["dec"]}) >= 2 and len({d[0] for d in general["dec"]}) == 2, general["dec"]


def test_general_scenes(slam, general):
    from slam_jl_amd.keypoint_set import keyframe_required
    S = len(GENERAL)
    ks = slam.KeypointSet(S, 1400)
    _fill(ks, general["streams"])
    T = np.tile(np.eye(4), (S, 1, 1)); T[:, :3, :3] = general["R"]
    sp = slam.stream_params(S, Tcw=T, cam=general["cam"], dist=DIST)
    before = [(ks.download(s), ks.download_keyframe(s)) for s in range(S)]
    cnt0 = ks.counts()
    got = {}
    for flags in (1, 3):
        got[flags] = ks.frame_stats(sp, flags, CELL0, (H0, W0))
        want = general["want"][flags]
        err = np.abs(got[flags][:, 6:] - want[:, 6:])
        print(f"flags {flags}: |mean - model| {err[:, 0].max():.3e}  |median - model| {err[:, 1].max():.3e} px")
        assert np.array_equal(got[flags][:, :6], want[:, :6]), (got[flags][:, :6], want[:, :6])
        assert err.max() <= 1e-9, err
    # two calls give the same bytes; the enqueue-only form into caller-owned HBM gives the same bytes as the synchronous one
    import torch
    again = ks.frame_stats(sp, 1, CELL0, (H0, W0))
    assert again.tobytes() == got[1].tobytes()
    dev = torch.full((S, 8), -1.0, dtype=torch.float64, device="cuda"); torch.cuda.synchronize()
    assert ks.frame_stats(sp, 1, CELL0, (H0, W0), fetch=False, stats_dev_ptr=dev.data_ptr()) is None
    ks.ctx.synchronize()
    assert dev.cpu().numpy().tobytes() == got[1].tobytes()
    assert ks.frame_stats(sp, 1, CELL0, (H0, W0), fetch=False) is None                          # into the set's own buffer: nothing to read, must not fail
    # the lists are only read
    assert np.array_equal(ks.counts(), cnt0)
    for s in range(S):
        d, (k, f) = ks.download(s), ks.download_keyframe(s)
        for key in d:
            assert np.array_equal(d[key], before[s][0][key]), (s, key)
        assert np.array_equal(k, before[s][1][0]) and np.array_equal(f, before[s][1][1])
    # the decision on the device's statistics is the model's
    g = np.array([x[3:] for x in GENERAL])
    req, rule = keyframe_required(got[1], g[:, 0], g[:, 1], g[:, 2], slam.Params(max_nb_keypoints=MAXKP))
    assert req.tolist() == [d[0] for d in general["dec"]] and rule.tolist() == [d[1] for d in general["dec"]], (req, rule, general["dec"])
    # the mean with compensation over all observed keypoints IS compute_pose_5pt!'s average parallax (same terms, same order); min_parallax
    # above every scene: the call returns before its RANSAC and removes nothing
    _, st5, _, par, cnt = ks.compute_pose_5pt(sp, min_parallax=1e9, iters=8, seed=1)
    print(f"|mean - compute_pose_5pt parallax| {np.abs(par - got[1][:, 6]).max():.3e} px")
    assert np.abs(par - got[1][:, 6]).max() <= 1e-9 and not st5.any() and np.array_equal(cnt, cnt0)
    ks.close()


def test_argument_errors_launch_nothing(slam, ks5):
    import ctypes as C
    from slam_jl_amd import _lib as L
    c = ks5.ctx
    sp = slam.stream_params(5, cam=CAM1, dist=NODIST)
    ks5.upload(0, np.array([[3.0, 4.0]]), np.zeros(1, bool))
    out = np.full((5, 8), -5.0)
    call = lambda p, flags, cell, h, w: c.lib.slam_kpset_frame_stats(c.h, ks5.h, p, flags, cell, h, w, None, L.ptr(out))
    for args in ((L.ptr(sp), 1, 0, 370, 1226), (L.ptr(sp), 1, -35, 370, 1226), (L.ptr(sp), 1, 35, 0, 1226), (L.ptr(sp), 1, 35, 370, 0), (None, 1, 35, 370, 1226),
                 (L.ptr(sp), 4, 35, 370, 1226), (L.ptr(sp), 1, 1, 1080, 1920)):                  # (the last: more cells than the kernel's bitmap)
        assert call(*args) == -1 and (out == -5.0).all(), args
    assert c.lib.slam_kpset_frame_stats(c.h, None, L.ptr(sp), 1, 35, 370, 1226, None, L.ptr(out)) == -1
    with pytest.raises(slam.SlamHipError):
        ks5.frame_stats(sp, 1, 0, (370, 1226))
    assert call(L.ptr(sp), 1, 35, 370, 1226) == 0 and out[0, 0] == 1.0                          # and the set still works
